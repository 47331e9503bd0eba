// The input pipeline on the device: decoded 8-bit RGB -> fp32 NHWC in the loader's colour space, with image.scale and the reference's
// augmentation in front, from host batches or gathered out of a resident set.  Bit for bit what dataset.py computes in numpy.
#include "common.h"

namespace {
// NN_UTILS.rgbToColorSpace / toRgb (utils/nn_utils.lua:188-249) for one pixel.  'y' is the reference's own weighting (:253-277); 'yuv' and
// 'hsl' are image.rgb2yuv / rgb2hsl and back [upstream, recalled: the formulas and constants of lua/image.lua:152-186].  Every operation
// is a single correctly rounded fp32 one in the order written (no fma, __fdiv_rn for the quotients): dataset.rgb2yuv / rgb2hsl and
// nn_utils.yuv2rgb / hsl2rgb restate the same sequences in numpy and agree with these bit for bit.
enum { CS_RGB = 0, CS_Y = 1, CS_YUV = 2, CS_HSL = 3 };
// one pixel of the loader's output: three planes, one for 'y'
__device__ __forceinline__ void store_colorspace(float* dst, long i, float r, float g, float b, int cs) {
#pragma clang fp contract(off)   // no fma: the same products and sums the numpy loader rounds one by one
    if (cs == CS_RGB) { dst[3 * i] = r; dst[3 * i + 1] = g; dst[3 * i + 2] = b; }
    else if (cs == CS_Y) {
        const float t0 = 0.21f * r, t1 = 0.72f * g, t2 = 0.07f * b;   // z = ((0 + .21 r) + .72 g) + .07 b (nn_utils.lua:268-270)
        dst[i] = (t0 + t1) + t2;
    } else if (cs == CS_YUV) {
        const float y0 = 0.299f * r, y1 = 0.587f * g, y2 = 0.114f * b;
        const float u0 = -0.14713f * r, u1 = 0.28886f * g, u2 = 0.436f * b;
        const float v0 = 0.615f * r, v1 = 0.51499f * g, v2 = 0.10001f * b;
        dst[3 * i] = (y0 + y1) + y2; dst[3 * i + 1] = (u0 - u1) + u2; dst[3 * i + 2] = (v0 - v1) - v2;
    } else {
        const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
        const float sum = mx + mn, l = __fdiv_rn(sum, 2.f);
        float h = 0.f, s = 0.f;
        if (mx != mn) {
            const float d = mx - mn;
            s = l > 0.5f ? __fdiv_rn(d, (2.f - mx) - mn) : __fdiv_rn(d, sum);
            if (mx == r) h = __fdiv_rn(g - b, d) + (g < b ? 6.f : 0.f);
            else if (mx == g) h = __fdiv_rn(b - r, d) + 2.f;
            else h = __fdiv_rn(r - g, d) + 4.f;
            h = __fdiv_rn(h, 6.f);
        }
        dst[3 * i] = h; dst[3 * i + 1] = s; dst[3 * i + 2] = l;
    }
}
// image.hsl2rgb's helper (lua/image.lua:171-178); 1/6, 2/3 and 1/3 are the fp32 neighbours of the quotients
__device__ __forceinline__ float hsl_hue(float p, float q, float t) {
#pragma clang fp contract(off)
    const float sixth = (float)(1.0 / 6.0), two_thirds = (float)(2.0 / 3.0);
    if (t < 0.f) t += 1.f;
    if (t > 1.f) t -= 1.f;
    if (t < sixth) { const float a = (q - p) * 6.f, m = a * t; return p + m; }
    if (t < 0.5f) return q;
    if (t < two_thirds) { const float a = (q - p) * (two_thirds - t), m = a * 6.f; return p + m; }
    return p;
}
// the way back (NN_UTILS.toRgb, nn_utils.lua:188-220): the three planes of a 'yuv' or 'hsl' pixel -> r, g, b
__device__ __forceinline__ void colorspace_to_rgb(float a, float b, float c, int cs, float* rgb) {
#pragma clang fp contract(off)
    if (cs == CS_YUV) {
        const float rv = 1.13983f * c, gu = 0.39465f * b, gv = 0.58060f * c, bu = 2.03211f * b;
        rgb[0] = a + rv; rgb[1] = (a - gu) - gv; rgb[2] = a + bu;
    } else {
        const float h = a, s = b, l = c;
        if (s == 0.f) { rgb[0] = l; rgb[1] = l; rgb[2] = l; return; }
        const float third = (float)(1.0 / 3.0);
        const float ls = l * s;
        const float q = l < 0.5f ? l * (1.f + s) : (l + s) - ls;
        const float p = 2.f * l - q;
        rgb[0] = hsl_hue(p, q, h + third); rgb[1] = hsl_hue(p, q, h); rgb[2] = hsl_hue(p, q, h - third);
    }
}
// fp32 NHWC pixels that are on the device already (a pool held as rgb; images on their way to a grid).  One lane per pixel; it reads
// its three floats before it writes, so src == dst is fine whenever three planes come out
__global__ void colorspace_convert_k(const float* src, float* dst, long npix, int from, int to) {
    CG_GRID_STRIDE(i, npix) {
        const float a = src[3 * i], b = src[3 * i + 1], c = src[3 * i + 2];
        if (from == CS_RGB) store_colorspace(dst, i, a, b, c, to);
        else {
            float rgb[3];
            colorspace_to_rgb(a, b, c, from, rgb);
            dst[3 * i] = rgb[0]; dst[3 * i + 1] = rgb[1]; dst[3 * i + 2] = rgb[2];
        }
    }
}
// one lane per pixel; every operation correctly rounded on its own, like the numpy loader's
__global__ void images_u8_to_f32_k(const unsigned char* __restrict__ src, float* __restrict__ dst, long npix, int cs) {
#pragma clang fp contract(off)   // no fma: the same three products and two sums the numpy loader rounds one by one
    CG_GRID_STRIDE(i, npix) {
        const float r = __fdiv_rn((float)src[3 * i], 255.f), g = __fdiv_rn((float)src[3 * i + 1], 255.f), b = __fdiv_rn((float)src[3 * i + 2], 255.f);
        store_colorspace(dst, i, r, g, b, cs);
    }
}

// image.load -> image.scale -> NN_UTILS.rgbToColorSpace (dataset.lua:123-131,166) on the device: 8-bit RGB as decoded, [N][Hs][Ws][3]
// -> fp32 NHWC [N][Hd][Wd][C].  image.scale's default mode is the torch `image` rock's separable 'bilinear' [upstream, recalled:
// generic/image.c scaleLinear_rowcol]: first every row to the target width, then every column to the target height, each pass in
// fp32.  One axis, source length Ls, target length Ld, scale = (float)Ls / Ld (down) or (float)(Ls-1)/(Ld-1) (up):
//   Ld <  Ls: box average with fractional ends - out[d] = (w0 s[i0] + s[i0+1] + ... + s[i1-1] + f1 s[i1]) / (w0 + ... + f1), where
//             [i0 + (1-w0), i1 + f1) = [d scale, (d+1) scale) and the last term is dropped when i1 == Ls;
//   Ld >  Ls: out[d] = (1-f) s[i] + f s[i+1] with i + f = d scale, the last sample copied;          Ld == Ls: a copy.
// Every operation is a single correctly rounded fp32 one in the order of that loop (no fma), so the host loader's numpy restatement
// and this kernel agree bit for bit.  One lane per output element.
// s[k - base] holds source sample k for the few k this target sample touches
__device__ __forceinline__ float scale_axis(const float* w, int base, int Ls, int Ld, int d) {
#pragma clang fp contract(off)
#define s(k) w[(k) - base]
    if (Ld == Ls) return s(d);
    if (Ld > Ls) {
        if (d == Ld - 1 || Ls == 1) return s(Ls == 1 ? 0 : Ls - 1);
        const float scale = __fdiv_rn((float)(Ls - 1), (float)(Ld - 1));
        float sf = (float)d * scale;
        const int si = (int)sf;
        sf -= (float)si;
        const float a = (1.f - sf) * s(si), b = sf * s(si + 1);
        return a + b;
    }
    const float scale = __fdiv_rn((float)Ls, (float)Ld);
    float f0 = (float)d * scale;
    int i0 = (int)f0;
    f0 -= (float)i0;
    if (d == 0) { i0 = 0; f0 = 0.f; }
    float f1 = (float)(d + 1) * scale;
    const int i1 = (int)f1;
    f1 -= (float)i1;
    float acc = (1.f - f0) * s(i0), n = 1.f - f0;
    for (int si = i0 + 1; si < i1; ++si) { acc += s(si); n += 1.f; }
    if (i1 < Ls) { const float t = f1 * s(i1); acc += t; n += f1; }
    return __fdiv_rn(acc, n);
#undef s
}
// the footprint of target sample d on that axis: scale_axis reads the source samples lo..hi and no other.  Down: the box's first and
// last sample, the last clipped to the axis (d == 0 starts at 0 whatever the product rounds to); up: the two taps, the last target
// sample (and a one-sample source) on the last sample alone; equal: d itself.  The same quotient and products as scale_axis
__device__ __forceinline__ void scale_footprint(int Ls, int Ld, int d, int* lo, int* hi) {
#pragma clang fp contract(off)
    *lo = d; *hi = d;
    if (Ld < Ls) {
        const float scale = __fdiv_rn((float)Ls, (float)Ld);
        *lo = d == 0 ? 0 : (int)((float)d * scale);
        *hi = min(Ls - 1, (int)((float)(d + 1) * scale));
    } else if (Ld > Ls) {
        const float scale = __fdiv_rn((float)(Ls - 1), (float)(Ld - 1));
        *lo = (d == Ld - 1 || Ls == 1) ? Ls - 1 : (int)((float)d * scale);
        *hi = min(Ls - 1, *lo + 1);
    }
}
// output element i = (n, oy, ox) of the pool from the one source image `im`: both scaling kernels' whole arithmetic
__device__ __forceinline__ void scale_pixel(const unsigned char* __restrict__ im, float* __restrict__ dst, long i, int ox, int oy, int Hs, int Ws,
                                            int Hd, int Wd, int cs) {
#pragma clang fp contract(off)
    int y0, y1;   // vertical footprint of this output row (the second pass reads the first pass's fp32 rows)
    scale_footprint(Hs, Hd, oy, &y0, &y1);
    float rgb[3];
    for (int c = 0; c < 3; ++c) {
        float col[8];   // first pass at column ox for the source rows y0..y1 (<= 8 rows: down-scaling factors up to 6)
        for (int y = y0; y <= y1 && y - y0 < 8; ++y) {
            int x0, x1;   // horizontal footprint of ox in row y
            scale_footprint(Ws, Wd, ox, &x0, &x1);
            float row[8];
            for (int x = x0; x <= x1 && x - x0 < 8; ++x) row[x - x0] = __fdiv_rn((float)im[((long)y * Ws + x) * 3 + c], 255.f);
            col[y - y0] = scale_axis(row, x0, Ws, Wd, ox);
        }
        rgb[c] = scale_axis(col, y0, Hs, Hd, oy);
    }
    store_colorspace(dst, i, rgb[0], rgb[1], rgb[2], cs);
}
// output pixel i of an image that has no source (a gathered index outside the set): every plane zero
__device__ __forceinline__ void store_zero_pixel(float* dst, long i, int cs) {
    if (cs == CS_Y) dst[i] = 0.f;
    else { dst[3 * i] = 0.f; dst[3 * i + 1] = 0.f; dst[3 * i + 2] = 0.f; }
}
__global__ void images_u8_scale_k(const unsigned char* __restrict__ src, float* __restrict__ dst, int N, int Hs, int Ws, int Hd, int Wd, int cs) {
    const long total = (long)N * Hd * Wd;
    CG_GRID_STRIDE(i, total) {
        const int ox = (int)(i % Wd), oy = (int)((i / Wd) % Hd);
        const long n = i / ((long)Wd * Hd);
        scale_pixel(src + n * (long)Hs * Ws * 3, dst, i, ox, oy, Hs, Ws, Hd, Wd, cs);
    }
}
// The same over a set that stays resident in device memory (dataset.ResidentSet): image n of the pool comes from set[idx[n]], read in
// place - the gathered bytes are never copied.  The set may exceed 2^31 bytes: the image's base is a 64-bit product.
__global__ void images_u8_gather_scale_k(const unsigned char* __restrict__ set, long M, const int32_t* __restrict__ idx, float* __restrict__ dst,
                                         int N, int Hs, int Ws, int Hd, int Wd, int cs) {
    const long total = (long)N * Hd * Wd;
    CG_GRID_STRIDE(i, total) {
        const int ox = (int)(i % Wd), oy = (int)((i / Wd) % Hd);
        const long n = i / ((long)Wd * Hd);
        const long m = idx[n];
        if (m < 0 || m >= M) store_zero_pixel(dst, i, cs);
        else scale_pixel(set + m * ((long)Hs * Ws * 3), dst, i, ox, oy, Hs, Ws, Hd, Wd, cs);
    }
}

// The same with the reference's augmentation in front (dataset/dataset.py:284-306 with the matrices of ImageAugmenter.py:160-190;
// semantics under cg_images_u8_augment_to_f32 and cg_images_u8_augment_window_to_f32 in catgan.h, numpy restatement
// dataset.augment_images).  One workgroup per image.  Phase 1 leaves the pixel stage p (flip, brightness, noise, clip) of the whole
// padded source image in the LDS as fp32, [Hp][Wp][3], so that a noise value is hashed once and not once per bilinear tap of every
// box-filter sample that touches it.  Phase 2 is images_u8_scale_k's walk over the window [margin, margin + Hs) x [margin, margin + Ws),
// one lane per output element, whose source samples are the four warp taps out of the LDS; the margin is what a tap may reach before
// it is clamped.  margin == 0: the window is the image, the form without a margin.
using cg::augment_noise;
using cg::warp_taps;
// image n of the pool (this workgroup's) from the one source image `im`: both augmentation kernels' whole arithmetic.  n, not the
// image's place in its set, numbers the noise counters.  desc == nullptr: the identity draw (1 0 0 0 1 0 1 0) for every image
__device__ __forceinline__ void augment_image(const unsigned char* __restrict__ im, long n, float* __restrict__ dst, int Hp, int Wp, int margin,
                                              int Hd, int Wd, int cs, const float* __restrict__ desc, float sigma, uint64_t seed,
                                              uint64_t offset) {
#pragma clang fp contract(off)
    extern __shared__ float aug_p[];   // [Hp][Wp][3]
    float m00 = 1.f, m01 = 0.f, m02 = 0.f, m10 = 0.f, m11 = 1.f, m12 = 0.f, bright = 1.f;
    bool flip = false;
    if (desc) {
        const float* d = desc + n * 8;
        m00 = d[0]; m01 = d[1]; m02 = d[2]; m10 = d[3]; m11 = d[4]; m12 = d[5]; bright = d[6];
        flip = d[7] != 0.f;
    }
    const int Hs = Hp - 2 * margin, Ws = Wp - 2 * margin;
    const int row3 = Wp * 3, nsrc = Hp * row3;
    for (int k = threadIdx.x; k < nsrc; k += 256) {
        const int y = k / row3, r = k - y * row3, x = r / 3, c = r - x * 3;
        const int xf = flip ? Wp - 1 - x : x;
        float v = __fdiv_rn((float)im[y * row3 + xf * 3 + c], 255.f) * bright;
        if (sigma != 0.f) {
            const float t = sigma * augment_noise(seed, offset + 3ull * (uint64_t)(n * nsrc + k));
            v += t;
        }
        v = v < 0.f ? 0.f : v;
        aug_p[k] = v > 1.f ? 1.f : v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < Hd * Wd; e += 256) {
        const int ox = e % Wd, oy = e / Wd;
        int y0, y1, x0, x1;   // the footprints of images_u8_scale_k
        scale_footprint(Hs, Hd, oy, &y0, &y1);
        scale_footprint(Ws, Wd, ox, &x0, &x1);
        float col[3][8];   // first pass at column ox for the source rows y0..y1, per channel
        for (int y = y0; y <= y1 && y - y0 < 8; ++y) {
            float row[3][8];
            for (int x = x0; x <= x1 && x - x0 < 8; ++x) {
                const float X = (float)(x + margin), Y = (float)(y + margin);      // window sample (x, y) at its padded position
                const float ax = m00 * X, bx = m01 * Y, ay = m10 * X, by = m11 * Y;
                int tx0, tx1, ty0, ty1;
                float fx, fy;
                warp_taps((ax + bx) + m02, Wp, &tx0, &tx1, &fx);
                warp_taps((ay + by) + m12, Hp, &ty0, &ty1, &fy);
                const float gx = 1.f - fx, gy = 1.f - fy;
                const float *p00 = aug_p + ty0 * row3 + tx0 * 3, *p01 = aug_p + ty0 * row3 + tx1 * 3;
                const float *p10 = aug_p + ty1 * row3 + tx0 * 3, *p11 = aug_p + ty1 * row3 + tx1 * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float ta = gx * p00[c], tb = fx * p01[c], ba = gx * p10[c], bb = fx * p11[c];
                    const float top = ta + tb, bot = ba + bb;
                    const float wa = gy * top, wb = fy * bot;
                    row[c][x - x0] = wa + wb;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c][y - y0] = scale_axis(row[c], x0, Ws, Wd, ox);
        }
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = scale_axis(col[c], y0, Hs, Hd, oy);
        store_colorspace(dst, n * (long)Hd * Wd + e, rgb[0], rgb[1], rgb[2], cs);
    }
}
__global__ void __launch_bounds__(256) images_u8_augment_k(const unsigned char* __restrict__ src, float* __restrict__ dst, int Hp, int Wp,
                                                            int margin, int Hd, int Wd, int cs, const float* __restrict__ desc, float sigma,
                                                            uint64_t seed, uint64_t offset) {
    const long n = blockIdx.x;
    augment_image(src + n * (long)Hp * Wp * 3, n, dst, Hp, Wp, margin, Hd, Wd, cs, desc, sigma, seed, offset);
}
// the gather form (images_u8_gather_scale_k's addressing): the whole workgroup takes the same branch, so the barrier inside stays uniform
__global__ void __launch_bounds__(256) images_u8_gather_augment_k(const unsigned char* __restrict__ set, long M, const int32_t* __restrict__ idx,
                                                                   float* __restrict__ dst, int Hp, int Wp, int margin, int Hd, int Wd, int cs,
                                                                   const float* __restrict__ desc, float sigma, uint64_t seed, uint64_t offset) {
    const long n = blockIdx.x;
    const long m = idx[n];
    if (m < 0 || m >= M) {
        for (int e = threadIdx.x; e < Hd * Wd; e += 256) store_zero_pixel(dst, n * (long)Hd * Wd + e, cs);
        return;
    }
    augment_image(set + m * ((long)Hp * Wp * 3), n, dst, Hp, Wp, margin, Hd, Wd, cs, desc, sigma, seed, offset);
}

}  // namespace

extern "C" {

int cg_images_u8_to_f32(void* stream, const unsigned char* src, float* dst, long npixels, int colorspace) {
    CG_REQUIRE(src && dst && npixels > 0 && colorspace >= CS_RGB && colorspace <= CS_HSL, "cg_images_u8_to_f32: bad arguments");
    CG_EW_LAUNCH(images_u8_to_f32_k, npixels, src, dst, npixels, colorspace); return 0;
}

// the two scaling entry points' checks; `given`: whether what the form has beyond the sizes, its pointers and the set's size, is there
static int scale_check(const char* who, bool given, int N, int Hs, int Ws, int Hd, int Wd, int colorspace) {
    CG_REQUIRE(given && N > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && colorspace >= CS_RGB && colorspace <= CS_HSL, "%s: bad arguments", who);
    CG_REQUIRE(Hs <= 6 * Hd && Ws <= 6 * Wd, "%s: down-scaling by more than 6 is not supported", who);
    return 0;
}
int cg_images_u8_scale_to_f32(void* stream, const unsigned char* src, float* dst, int N, int Hs, int Ws, int Hd, int Wd, int colorspace) {
    if (int rc = scale_check("cg_images_u8_scale_to_f32", src && dst, N, Hs, Ws, Hd, Wd, colorspace)) return rc;
    const long total = (long)N * Hd * Wd;
    CG_EW_LAUNCH(images_u8_scale_k, total, src, dst, N, Hs, Ws, Hd, Wd, colorspace); return 0;
}

// the pixel stage of one image in the LDS: 64 x 64 sources take 48 KB (three workgroups per CU); above 64 KB a kernel has to ask.  Both
// augmentation kernels ask together, so one record per thread serves them
static int augment_lds(const char* who, int Hp, int Wp, long* lds_out) {
    static thread_local int lds_dev = -1, lds_max = 0, lds_asked = 0;
    int dev = 0;
    CG_HIP(hipGetDevice(&dev));
    if (dev != lds_dev) {
        CG_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        lds_dev = dev; lds_asked = 0;
    }
    const long lds = (long)Hp * Wp * 3 * sizeof(float);
    CG_REQUIRE(lds <= lds_max, "%s: a %d x %d source needs %ld bytes of LDS, the device has %d per workgroup", who, Wp, Hp, lds, lds_max);
    if (lds > 65536 && lds > lds_asked) {
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(images_u8_augment_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(images_u8_gather_augment_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        lds_asked = lds_max;
    }
    *lds_out = lds;
    return 0;
}
// the four augmentation entry points' checks beyond their pointers, and the LDS: the shrink limit is the window's, the LDS the padded
// array's.  The forms without a margin pass 0 and insist on a descriptor buffer themselves
static int augment_check(const char* who, int N, int Hp, int Wp, int margin, int Hd, int Wd, int colorspace, float noise_std, long* lds_out) {
    CG_REQUIRE(N > 0 && Hp > 0 && Wp > 0 && Hd > 0 && Wd > 0 && colorspace >= CS_RGB && colorspace <= CS_HSL && noise_std >= 0.f,
               "%s: bad arguments", who);
    CG_REQUIRE(margin >= 0 && margin <= (std::min(Hp, Wp) - 1) / 2, "%s: a margin of %d leaves no window in a %d x %d padded image", who,
               margin, Wp, Hp);
    CG_REQUIRE(Hp - 2 * margin <= 6 * Hd && Wp - 2 * margin <= 6 * Wd, "%s: down-scaling by more than 6 is not supported", who);
    return augment_lds(who, Hp, Wp, lds_out);
}
// ... and their launch, one workgroup per image: idx != nullptr is the gather form out of a set of M images
static int augment_launch(const char* who, void* stream, const unsigned char* src, long M, const int32_t* idx, float* dst, int N, int Hp, int Wp,
                          int margin, int Hd, int Wd, int colorspace, const float* desc, float noise_std, uint64_t seed, uint64_t offset) {
    long lds = 0;
    if (int rc = augment_check(who, N, Hp, Wp, margin, Hd, Wd, colorspace, noise_std, &lds)) return rc;
    if (idx) hipLaunchKernelGGL(images_u8_gather_augment_k, dim3(N), dim3(256), (size_t)lds, cg::S(stream), src, M, idx, dst, Hp, Wp, margin, Hd, Wd,
                                colorspace, desc, noise_std, seed, offset);
    else hipLaunchKernelGGL(images_u8_augment_k, dim3(N), dim3(256), (size_t)lds, cg::S(stream), src, dst, Hp, Wp, margin, Hd, Wd, colorspace, desc,
                            noise_std, seed, offset);
    CG_LAUNCH_CHECK();
    return 0;
}

int cg_images_u8_augment_window_to_f32(void* stream, const unsigned char* src, float* dst, int N, int Hp, int Wp, int margin, int Hd, int Wd,
                                       int colorspace, const float* desc, float noise_std, uint64_t seed, uint64_t offset) {
    CG_REQUIRE(src && dst, "cg_images_u8_augment_window_to_f32: bad arguments");
    return augment_launch("cg_images_u8_augment_window_to_f32", stream, src, 0, nullptr, dst, N, Hp, Wp, margin, Hd, Wd, colorspace, desc, noise_std,
                          seed, offset);
}
int cg_images_u8_augment_to_f32(void* stream, const unsigned char* src, float* dst, int N, int Hs, int Ws, int Hd, int Wd, int colorspace,
                                const float* desc, float noise_std, uint64_t seed, uint64_t offset) {
    CG_REQUIRE(src && dst && desc, "cg_images_u8_augment_to_f32: bad arguments");
    return augment_launch("cg_images_u8_augment_to_f32", stream, src, 0, nullptr, dst, N, Hs, Ws, 0, Hd, Wd, colorspace, desc, noise_std, seed, offset);
}

int cg_images_u8_gather_scale_to_f32(void* stream, const unsigned char* set, long M, const int32_t* idx, float* dst, int N, int Hs, int Ws,
                                     int Hd, int Wd, int colorspace) {
    if (int rc = scale_check("cg_images_u8_gather_scale_to_f32", set && idx && dst && M > 0, N, Hs, Ws, Hd, Wd, colorspace)) return rc;
    const long total = (long)N * Hd * Wd;
    CG_EW_LAUNCH(images_u8_gather_scale_k, total, set, M, idx, dst, N, Hs, Ws, Hd, Wd, colorspace); return 0;
}

int cg_images_u8_gather_augment_window_to_f32(void* stream, const unsigned char* set, long M, const int32_t* idx, float* dst, int N, int Hp,
                                              int Wp, int margin, int Hd, int Wd, int colorspace, const float* desc, float noise_std,
                                              uint64_t seed, uint64_t offset) {
    CG_REQUIRE(set && idx && dst && M > 0, "cg_images_u8_gather_augment_window_to_f32: bad arguments");
    return augment_launch("cg_images_u8_gather_augment_window_to_f32", stream, set, M, idx, dst, N, Hp, Wp, margin, Hd, Wd, colorspace, desc,
                          noise_std, seed, offset);
}
int cg_images_u8_gather_augment_to_f32(void* stream, const unsigned char* set, long M, const int32_t* idx, float* dst, int N, int Hs, int Ws,
                                       int Hd, int Wd, int colorspace, const float* desc, float noise_std, uint64_t seed, uint64_t offset) {
    CG_REQUIRE(set && idx && dst && desc && M > 0, "cg_images_u8_gather_augment_to_f32: bad arguments");
    return augment_launch("cg_images_u8_gather_augment_to_f32", stream, set, M, idx, dst, N, Hs, Ws, 0, Hd, Wd, colorspace, desc, noise_std, seed,
                          offset);
}
int cg_colorspace_convert(void* stream, const float* src, float* dst, long npixels, int from, int to) {
    CG_REQUIRE(src && dst && npixels > 0, "cg_colorspace_convert: bad arguments");
    CG_REQUIRE((from == CS_RGB && to >= CS_Y && to <= CS_HSL) || ((from == CS_YUV || from == CS_HSL) && to == CS_RGB),
               "cg_colorspace_convert: unsupported pair %d -> %d (rgb -> y | yuv | hsl, yuv | hsl -> rgb)", from, to);
    CG_REQUIRE(to != CS_Y || src != dst, "cg_colorspace_convert: rgb -> y cannot run in place (one plane out of three)");
    CG_EW_LAUNCH(colorspace_convert_k, npixels, src, dst, npixels, from, to); return 0;
}
}  // extern "C"
