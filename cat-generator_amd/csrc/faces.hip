// The reference's offline face extraction (dataset/generate_dataset.py:53-91 with dataset/dataset.py:152-181, 191-239, 127-139) for its
// un-augmented variant, on the device: per face, the rotation-removing warp of the face rectangle out of the decoded source image and
// Pillow's 8-bit bilinear resampling of that rectangle to out x out.  Semantics under cg_faces_u8_extract in catgan.h; the numpy
// restatement is faces.extract_faces_np.  Two kernels:
//   faces_warp_hpass_k  one workgroup per band of rectangle rows of one face: the rows are warped into the LDS as bytes (only rectangle
//                       pixels are ever warped - the warp is pointwise, so this equals rotating the whole image and cropping), then
//                       the horizontal pass runs out of the LDS against the face's taps into tmp[face][row][out][3];
//   faces_vpass_k       the vertical pass, consecutive lanes along (ox, c): loads and stores are contiguous.
// Nothing but tmp (Hr out 3 bytes per face) goes to memory between them.  The warp is fp32 with every operation rounded once, the
// resampling is integer arithmetic alone: no floating point decides a tap on the device.
//
// cg_faces_u8_extract_variants makes the tool's augmented variants (generate_dataset.py:62-73, dataset.py:191-230, 284-308, 145-150)
// from the PADDED full-resolution crop; the numpy restatement is faces.variants_np.  Three kernels in front of the same vertical pass:
//   faces_crop_k        the in-image window of each face's padded crop, warped and truncated, into crop[face] [Hp][Wp][3];
//   faces_median_k      np.pad(mode="median") for the sides that leave the image, one wave per line: a 3 x 256 histogram in the LDS
//                       (integer adds, which commute), the two middle order statistics by a prefix walk, their mean rounded half to
//                       even; launched over axis 0 and then over axis 1 (all rows, those just filled included), and only over the
//                       lines of faces that have such a side;
//   faces_variant_hpass_k  one workgroup per (band of window rows, variant): the second warp, whose taps read the pixel stage
//                       (flip, brightness, noise, clip, truncation) evaluated on the fly out of the crop - the noise is keyed by the
//                       source position, so a tap shared by two outputs agrees - then the horizontal pass out of the LDS.
//
// cg_faces_u8_extract_padded makes the padded faces of generate_dataset.py --margin: the whole padded crop of each face, its pad its
// own (faces_crop_k and faces_median_k read a pad per face; the variants pass their one scalar), resized.  The numpy restatement is
// faces.padded_face_np.  One kernel between the crops and the same vertical pass:
//   faces_crop_hpass_k  one workgroup per band of crop rows: the finished rows are copied into the LDS byte for byte (no warp - an
//                       identity warp would re-quantise through (u8)((v / 255) 255), which is not v for every byte), then the
//                       horizontal pass out of the LDS against the tables of the PADDED sides.
#include <vector>
#include "common.h"

namespace cg {
namespace {

constexpr int kBandBytes = 32768;   // the LDS a workgroup keeps its warped rows in
constexpr int kBandRowsMax = 16;
constexpr int kGeom = 8;            // int32 per face: Hs Ws y0 x0 Hr Wr kx ky
// rows per band of a rectangle Wr wide: >= 2 for every Wr <= 4096
__host__ __device__ inline int band_rows(int Wr) {
    const int r = kBandBytes / (Wr * 3);
    return r > kBandRowsMax ? kBandRowsMax : r;
}
// Pillow's ksize of one axis (Resample.c precompute_coeffs, bilinear support 1): 2 ceil(max(in / out, 1)) + 1
inline int resample_ksize(int in, int out) { return 2 * ((std::max(in, out) + out - 1) / out) + 1; }
__device__ __forceinline__ unsigned char clip8(int ss) {
    const int v = ss >> 22;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One pixel of the fp32 restatement of tf.warp (order 1, edge replication): the source position of the output pixel (xf, yf) under the
// inverse map m, its four taps inside W x H, px(y, x, c) the 8-bit sample there -> o[c] = (u8)(w 255), truncated (dataset.py:174)
template <class Px>
__device__ __forceinline__ void warp_pixel(const float* __restrict__ unit, const float* __restrict__ m, float xf, float yf, int W, int H,
                                           const Px& px, unsigned char* o) {
#pragma clang fp contract(off)
    const float ax = m[0] * xf, bx = m[1] * yf, ay = m[3] * xf, by = m[4] * yf;
    int tx0, tx1, ty0, ty1;
    float fx, fy;
    warp_taps((ax + bx) + m[2], W, &tx0, &tx1, &fx);
    warp_taps((ay + by) + m[5], H, &ty0, &ty1, &fy);
    const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ta = gx * unit[px(ty0, tx0, c)], tb = fx * unit[px(ty0, tx1, c)];
        const float ba = gx * unit[px(ty1, tx0, c)], bb = fx * unit[px(ty1, tx1, c)];
        const float top = ta + tb, bot = ba + bb;
        const float wa = gy * top, wb = fy * bot;
        o[c] = (unsigned char)(int)((wa + wb) * 255.f);
    }
}
// the samples of a decoded image [H][W][3]
struct ImagePx {
    const unsigned char* im;
    int row3;
    __device__ __forceinline__ int operator()(int y, int x, int c) const { return im[y * row3 + x * 3 + c]; }
};
// the samples of a variant's pixel stage over the padded crop P [Hp][Wp][3] (dataset.py:284-304, re-quantised as the tool does):
// q = (u8) clip(fl(fl(P[y][flip ? Wp-1-x : x][c] bright) + fl(sigma z)), 0, 255), z keyed by the position on the array the warp reads
struct VariantPx {
    const unsigned char* crop;
    int Wp;
    float bright, sigma;
    bool flip;
    uint64_t seed, base;
    __device__ __forceinline__ int operator()(int y, int x, int c) const {
#pragma clang fp contract(off)
        const int j = (y * Wp + x) * 3 + c;
        float v = (float)crop[(y * Wp + (flip ? Wp - 1 - x : x)) * 3 + c] * bright;
        if (sigma != 0.f) {
            const float t = sigma * augment_noise(seed, base + 3ull * (uint64_t)j);
            v += t;
        }
        v = !(v >= 0.f) ? 0.f : (v > 255.f ? 255.f : v);
        return (int)v;
    }
};
// u8 / 255, divided once per workgroup and not twelve times per pixel
__device__ __forceinline__ void fill_unit(float* unit) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) unit[i] = __fdiv_rn((float)i, 255.f);
}
// the face whose blocks hold b: start[f] <= b < start[f + 1], start [N + 1] ascending
__device__ __forceinline__ int owner(const int32_t* __restrict__ start, int N, int b) {
    int f = 0, hi = N;
    while (hi - f > 1) {
        const int mid = (f + hi) >> 1;
        if (start[mid] <= b) f = mid; else hi = mid;
    }
    return f;
}
// the band of rows that block b works on: its face, its first row and its rows, for faces whose geometry rows hold (H, W) at [4], [5]
struct Band {
    int f, r0, nr;
};
__device__ __forceinline__ Band band_of(const int32_t* __restrict__ band_start, const int32_t* __restrict__ geom, int N, int b) {
    const int f = owner(band_start, N, b);
    const int H = geom[(long)f * kGeom + 4], R = band_rows(geom[(long)f * kGeom + 5]), r0 = (b - band_start[f]) * R;
    return {f, r0, min(R, H - r0)};
}
// the horizontal pass of nr warped rows [nr][Wr][3] out of the LDS against one table (tb: [out][2] (xmin, count), then [out][kx] taps)
__device__ __forceinline__ void hpass_band(const unsigned char* band, int nr, int Wr, const int32_t* __restrict__ tb, int kx, int out,
                                           unsigned char* __restrict__ trow) {
    const int32_t* tk = tb + 2 * out;
    const int o3 = out * 3;
    for (int e = threadIdx.x; e < nr * o3; e += 256) {
        const int r = e / o3, j = e - r * o3, ox = j / 3, c = j - ox * 3;
        const int xmin = tb[2 * ox], cnt = tb[2 * ox + 1];
        const unsigned char* p = band + (r * Wr + xmin) * 3 + c;
        const int32_t* k = tk + ox * kx;
        int ss = 1 << 21;
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) ss += (int)p[i * 3] * k[i];
        trow[e] = clip8(ss);
    }
}

__global__ void __launch_bounds__(256) faces_warp_hpass_k(const unsigned char* __restrict__ src, const uint64_t* __restrict__ src_off,
                                                          const int32_t* __restrict__ geom, const float* __restrict__ inv,
                                                          const int32_t* __restrict__ taps, const uint64_t* __restrict__ tap_off,
                                                          const int32_t* __restrict__ band_start, const uint64_t* __restrict__ tmp_off,
                                                          unsigned char* __restrict__ tmp, int N, int out) {
    __shared__ unsigned char band[kBandBytes];   // [rows][Wr][3]
    __shared__ float unit[256];
    fill_unit(unit);
    __syncthreads();
    const auto [f, r0, nr] = band_of(band_start, geom, N, blockIdx.x);
    const int32_t* g = geom + (long)f * kGeom;
    const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Wr = g[5], kx = g[6];
    const ImagePx px{src + src_off[f], Ws * 3};
    const float* m = inv + (long)f * 6;
    for (int e = threadIdx.x; e < nr * Wr; e += 256) {
        const int r = e / Wr, x = e - r * Wr;
        warp_pixel(unit, m, (float)(x0 + x), (float)(y0 + r0 + r), Ws, Hs, px, band + e * 3);
    }
    __syncthreads();
    hpass_band(band, nr, Wr, taps + tap_off[2 * f], kx, out, tmp + tmp_off[f] + (long)r0 * out * 3);
}

// the padded crop's in-image window (extract_rectangle, dataset.py:191-230, before its np.pad): kCropPixels pixels per workgroup.
// Face f's pad is pads[f], or pad_all for every face where pads is null
constexpr int kCropPixels = 1024;
__global__ void __launch_bounds__(256) faces_crop_k(const unsigned char* __restrict__ src, const uint64_t* __restrict__ src_off,
                                                    const int32_t* __restrict__ geom, const float* __restrict__ inv,
                                                    const int32_t* __restrict__ cblk_start, const uint64_t* __restrict__ crop_off,
                                                    unsigned char* __restrict__ crops, int N, const int32_t* __restrict__ pads,
                                                    int pad_all) {
    __shared__ float unit[256];
    fill_unit(unit);
    __syncthreads();
    const int b = blockIdx.x, f = owner(cblk_start, N, b);
    const int32_t* g = geom + (long)f * kGeom;
    const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], pad = pads ? pads[f] : pad_all;
    const int Wp = Wr + 2 * pad, top = max(0, pad - y0), left = max(0, pad - x0);
    const int Hwin = min(Hs - 1, y0 + Hr - 1 + pad) - (y0 - pad + top) + 1, Wwin = min(Ws - 1, x0 + Wr - 1 + pad) - (x0 - pad + left) + 1;
    const ImagePx px{src + src_off[f], Ws * 3};
    const float* m = inv + (long)f * 6;
    unsigned char* crop = crops + crop_off[f];
    const int e0 = (b - cblk_start[f]) * kCropPixels, e1 = min(e0 + kCropPixels, Hwin * Wwin);
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
        const int cy = top + e / Wwin, cx = left + e % Wwin;
        warp_pixel(unit, m, (float)(x0 - pad + cx), (float)(y0 - pad + cy), Ws, Hs, px, crop + ((long)cy * Wp + cx) * 3);
    }
}

// np.pad(mode="median") of one line, one wave per line.  axis 0: line = a column of the window, the median over the window's rows goes
// into that column's cells above and below; axis 1: line = a row of the whole crop, the median over the window's columns goes into the
// cells left and right.  The median of L bytes: the middle one, or the mean of the two middle ones rounded half to even.  The pad is
// faces_crop_k's.
__global__ void __launch_bounds__(64) faces_median_k(const int32_t* __restrict__ geom, const int32_t* __restrict__ line_face,
                                                     const int32_t* __restrict__ line_start, int nfaces, const uint64_t* __restrict__ crop_off,
                                                     unsigned char* __restrict__ crops, const int32_t* __restrict__ pads, int pad_all,
                                                     int axis) {
    __shared__ int hist[3][256];
    __shared__ int med[3];
    const int b = blockIdx.x, k = owner(line_start, nfaces, b), f = line_face[k], line = b - line_start[k];
    const int32_t* g = geom + (long)f * kGeom;
    const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], pad = pads ? pads[f] : pad_all;
    const int Hp = Hr + 2 * pad, Wp = Wr + 2 * pad;
    const int top = max(0, pad - y0), left = max(0, pad - x0);
    const int bottom = max(0, y0 + Hr - 1 + pad - (Hs - 1)), right = max(0, x0 + Wr - 1 + pad - (Ws - 1));
    // the line's first cell, the stride between its cells, the valid cells [lo, lo + L) and the line's length
    unsigned char* p = crops + crop_off[f] + (axis == 0 ? (long)(left + line) * 3 : (long)line * Wp * 3);
    const long stride = axis == 0 ? (long)Wp * 3 : 3;
    const int lo = axis == 0 ? top : left, n = axis == 0 ? Hp : Wp, L = n - lo - (axis == 0 ? bottom : right);
    for (int i = threadIdx.x; i < 3 * 256; i += 64) (&hist[0][0])[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < L * 3; i += 64) {
        const int r = i / 3, c = i - r * 3;
        atomicAdd(&hist[c][p[(lo + r) * stride + c]], 1);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k1 = (L - 1) >> 1, k2 = L >> 1;   // the two middle order statistics, the same one for odd L
        int cum = 0, a = -1, bb = -1;
        for (int v = 0; v < 256; ++v) {
            cum += hist[threadIdx.x][v];
            if (a < 0 && cum > k1) a = v;
            if (bb < 0 && cum > k2) bb = v;
        }
        const int t = a + bb;
        int mm = t >> 1;
        mm += (t & 1) & (mm & 1);
        med[threadIdx.x] = mm;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (n - L) * 3; i += 64) {
        const int r = i / 3, c = i - r * 3;
        p[(r < lo ? r : r + L) * stride + c] = (unsigned char)med[c];
    }
}

// A variant's window rows out of its face's padded crop: the pixel stage and the second warp into the LDS, then the horizontal pass
__global__ void __launch_bounds__(256) faces_variant_hpass_k(const unsigned char* __restrict__ crops, const uint64_t* __restrict__ crop_off,
                                                             const int32_t* __restrict__ geom, const float* __restrict__ desc,
                                                             const uint64_t* __restrict__ bases, const int32_t* __restrict__ taps,
                                                             const uint64_t* __restrict__ tap_off, const int32_t* __restrict__ band_start,
                                                             const uint64_t* __restrict__ tmp_off, unsigned char* __restrict__ tmp, int N, int A,
                                                             int pad, int out, float sigma, uint64_t seed) {
    __shared__ unsigned char band[kBandBytes];   // [rows][Wr][3]
    __shared__ float unit[256];
    fill_unit(unit);
    __syncthreads();
    const auto [f, r0, nr] = band_of(band_start, geom, N, blockIdx.x);
    const int a = blockIdx.y;
    const int32_t* g = geom + (long)f * kGeom;
    const int Hr = g[4], Wr = g[5], kx = g[6], Hp = Hr + 2 * pad, Wp = Wr + 2 * pad;
    const long item = (long)f * A + a;
    const float* d = desc + item * 8;
    const VariantPx px{crops + crop_off[f], Wp, d[6], sigma, d[7] != 0.f, seed, bases[item]};
    for (int e = threadIdx.x; e < nr * Wr; e += 256) {
        const int r = e / Wr, x = e - r * Wr;
        warp_pixel(unit, d, (float)(pad + x), (float)(pad + r0 + r), Wp, Hp, px, band + e * 3);
    }
    __syncthreads();
    hpass_band(band, nr, Wr, taps + tap_off[2 * f], kx, out, tmp + tmp_off[f] + ((long)a * Hr + r0) * out * 3);
}

// A band of rows of a finished crop through the horizontal pass.  pgeom holds the PADDED sides (Hp, Wp) and their ksizes where geom
// holds the rectangle's, so a band is nr Wp 3 contiguous bytes of the crop.  They are copied as they are, 16 bytes per lane between
// a head and a tail of single bytes; the LDS copy starts at the source's offset within 16 bytes, which aligns both sides alike.
__global__ void __launch_bounds__(256) faces_crop_hpass_k(const unsigned char* __restrict__ crops, const uint64_t* __restrict__ crop_off,
                                                          const int32_t* __restrict__ pgeom, const int32_t* __restrict__ taps,
                                                          const uint64_t* __restrict__ tap_off, const int32_t* __restrict__ band_start,
                                                          const uint64_t* __restrict__ tmp_off, unsigned char* __restrict__ tmp, int N, int out) {
    __shared__ __align__(16) unsigned char lds[kBandBytes + 16];   // [rows][Wp][3] from lds + (the source address & 15)
    const auto [f, r0, nr] = band_of(band_start, pgeom, N, blockIdx.x);
    const int Wp = pgeom[(long)f * kGeom + 5], kx = pgeom[(long)f * kGeom + 6], n = nr * Wp * 3;
    const unsigned char* p = crops + crop_off[f] + (long)r0 * Wp * 3;
    const int shift = (int)(reinterpret_cast<uintptr_t>(p) & 15), head = min((16 - shift) & 15, n), body = (n - head) >> 4;
    unsigned char* band = lds + shift;
    if ((int)threadIdx.x < head) band[threadIdx.x] = p[threadIdx.x];
    const uint4* p16 = reinterpret_cast<const uint4*>(p + head);
    uint4* b16 = reinterpret_cast<uint4*>(band + head);
    for (int i = threadIdx.x; i < body; i += 256) b16[i] = p16[i];
    for (int i = head + (body << 4) + threadIdx.x; i < n; i += 256) band[i] = p[i];
    __syncthreads();
    hpass_band(band, nr, Wp, taps + tap_off[2 * f], kx, out, tmp + tmp_off[f] + (long)r0 * out * 3);
}

// the vertical pass over N per_face items: item i belongs to face i / per_face, its rows follow its face's earlier items in tmp
__global__ void __launch_bounds__(256) faces_vpass_k(const unsigned char* __restrict__ tmp, const uint64_t* __restrict__ tmp_off,
                                                     const int32_t* __restrict__ geom, const int32_t* __restrict__ taps,
                                                     const uint64_t* __restrict__ tap_off, unsigned char* __restrict__ dst, int out,
                                                     int blocks_per_face, int per_face) {
    const int item = blockIdx.x / blocks_per_face, f = item / per_face;
    const int e = (blockIdx.x - item * blocks_per_face) * 256 + threadIdx.x;
    const int o3 = out * 3;
    if (e >= out * o3) return;
    const int oy = e / o3, j = e - oy * o3;
    const int Hr = geom[(long)f * kGeom + 4], ky = geom[(long)f * kGeom + 7];
    const int32_t* tb = taps + tap_off[2 * f + 1];
    const int32_t* k = tb + 2 * out + oy * ky;
    const int ymin = tb[2 * oy], cnt = tb[2 * oy + 1];
    const unsigned char* p = tmp + tmp_off[f] + ((long)(item - f * per_face) * Hr + ymin) * o3 + j;
    int ss = 1 << 21;
    for (int i = 0; i < cnt; ++i) ss += (int)p[(long)i * o3] * k[i];
    dst[(long)item * out * o3 + e] = clip8(ss);
}

// one axis' table at taps + off: inside the array, every sample's taps inside the side
int check_table(const char* who, const std::vector<int32_t>& taps, uint64_t off, int in, int out, int ksize, int f, const char* axis) {
    CG_REQUIRE(off <= taps.size() && (uint64_t)out * (2 + ksize) <= taps.size() - off,
               "%s: face %d: the %s tap table at %llu does not fit the %zu taps given", who, f, axis, (unsigned long long)off, taps.size());
    const int32_t* tb = taps.data() + off;
    for (int o = 0; o < out; ++o) {
        const long lo = tb[2 * o], cnt = tb[2 * o + 1];
        CG_REQUIRE(lo >= 0 && cnt >= 0 && cnt <= ksize && lo + cnt <= in,
                   "%s: face %d: %s sample %d reads [%ld, %ld) of a side of %d with ksize %d", who, f, axis, o, lo, lo + cnt, in, ksize);
    }
    return 0;
}

constexpr int kPadMax = 2048, kPaddedSideMax = 8192;   // band_rows(8192) is still 1; beyond 10922 it would be 0

// What the entry points take and check alike.  The descriptors are device arrays: they come back once, so that every limit is checked
// before anything is launched.  With `padded`, dpads [N] comes back too and the resampled sides - what ksize and the tap tables belong
// to - are the rectangle's enlarged by 2 pads[f]; without it pads stays empty and they are the rectangle's own
struct Faces {
    std::vector<int32_t> geom, taps, pads;
    std::vector<uint64_t> src_off, tap_off;
    int read(const char* who, hipStream_t s, const unsigned char* src, size_t src_bytes, const uint64_t* dsrc_off, const int32_t* dgeom,
             const float* inv, const int32_t* dtaps, size_t ntaps, const uint64_t* dtap_off, unsigned char* dst, int N, int out, void* workspace,
             const int32_t* dpads = nullptr, bool padded = false) {
        CG_REQUIRE(src && dsrc_off && dgeom && inv && dtaps && dtap_off && dst && workspace && (dpads || !padded), "%s: null pointer", who);
        CG_REQUIRE(N > 0 && N <= (1 << 20), "%s: N = %d is outside 1..2^20", who, N);
        CG_REQUIRE(out >= 8 && out <= 128, "%s: out = %d is outside 8..128", who, out);
        CG_REQUIRE(src_bytes > 0 && ntaps > 0 && ntaps <= (size_t)1 << 28, "%s: bad array lengths (%zu source bytes, %zu taps)", who, src_bytes, ntaps);
        geom.resize((size_t)N * kGeom), taps.resize(ntaps), src_off.resize(N), tap_off.resize((size_t)N * 2);
        CG_HIP(hipMemcpyAsync(geom.data(), dgeom, geom.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CG_HIP(hipMemcpyAsync(taps.data(), dtaps, taps.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CG_HIP(hipMemcpyAsync(src_off.data(), dsrc_off, src_off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        CG_HIP(hipMemcpyAsync(tap_off.data(), dtap_off, tap_off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (padded) {
            pads.resize(N);
            CG_HIP(hipMemcpyAsync(pads.data(), dpads, pads.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        CG_HIP(hipStreamSynchronize(s));
        for (int f = 0; f < N; ++f) {
            const int32_t* g = geom.data() + (size_t)f * kGeom;
            const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], kx = g[6], ky = g[7], pad = padded ? pads[f] : 0;
            CG_REQUIRE(Hs >= 8 && Hs <= 8192 && Ws >= 8 && Ws <= 8192, "%s: face %d: a %d x %d source is outside 8..8192", who, f, Ws, Hs);
            CG_REQUIRE(pad >= 0 && pad <= kPadMax, "%s: face %d: pad = %d is outside 0..%d", who, f, pad, kPadMax);
            // ahead of the rectangle's own limit, which with pad <= 2048 implies this one: the kernels' limit is the padded side
            CG_REQUIRE(!padded || ((long)Hr + 2 * pad <= kPaddedSideMax && (long)Wr + 2 * pad <= kPaddedSideMax),
                       "%s: face %d: a padded crop of %ld x %ld is beyond %d", who, f, (long)Wr + 2 * pad, (long)Hr + 2 * pad, kPaddedSideMax);
            CG_REQUIRE(Hr >= 8 && Hr <= 4096 && Wr >= 8 && Wr <= 4096, "%s: face %d: a %d x %d rectangle is outside 8..4096", who, f, Wr, Hr);
            CG_REQUIRE(y0 >= 0 && x0 >= 0 && (long)y0 + Hr <= Hs && (long)x0 + Wr <= Ws,
                       "%s: face %d: the rectangle (%d, %d) + %d x %d is not inside its %d x %d source", who, f, x0, y0, Wr, Hr, Ws, Hs);
            CG_REQUIRE(src_off[f] <= src_bytes && (uint64_t)Hs * Ws * 3 <= src_bytes - src_off[f],
                       "%s: face %d: its source at %llu does not fit the %zu bytes given", who, f, (unsigned long long)src_off[f], src_bytes);
            const int Hp = Hr + 2 * pad, Wp = Wr + 2 * pad;
            CG_REQUIRE(kx == resample_ksize(Wp, out) && ky == resample_ksize(Hp, out),
                       "%s: face %d: ksize (%d, %d) disagrees with the sides %d x %d -> %d, which need (%d, %d)", who, f, kx, ky, Wp, Hp, out,
                       resample_ksize(Wp, out), resample_ksize(Hp, out));
            if (int rc = check_table(who, taps, tap_off[2 * f], Wp, out, kx, f, "horizontal")) return rc;
            if (int rc = check_table(who, taps, tap_off[2 * f + 1], Hp, out, ky, f, "vertical")) return rc;
        }
        return 0;
    }
};

// pieces of a workspace head, each aligned to 16 bytes
struct Layout {
    size_t bytes = 0;
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes = (bytes + n + 15) / 16 * 16;
        return at;
    }
};

// The padded crops of a batch, face f's pad being pad_of(f): where each lies behind the workspace head, the crop kernel's block map and
// the lines of the two median launches.  reserve() takes their places in the head, plan() fills them, launch() enqueues the crop
// kernel and the median fills of the faces and axes that need one
struct Crops {
    size_t off_cblk = 0, off_ls[2] = {0, 0}, off_lf[2] = {0, 0}, off_cropoff = 0;
    long cblks = 0, lines[2] = {0, 0};
    int nlf[2] = {0, 0};
    uint64_t bytes = 0;   // every crop [Hp][Wp][3] from a multiple of 16
    void reserve(Layout& lay, int N) {
        off_cblk = lay.take((size_t)(N + 1) * 4);
        for (int a = 0; a < 2; ++a) off_ls[a] = lay.take((size_t)(N + 1) * 4);
        for (int a = 0; a < 2; ++a) off_lf[a] = lay.take((size_t)N * 4);
        off_cropoff = lay.take((size_t)N * 8);
    }
    template <class Pad>
    void plan(unsigned char* head, const int32_t* geom, int N, const Pad& pad_of) {
        auto i32 = [&](size_t off) { return reinterpret_cast<int32_t*>(head + off); };
        int32_t *cblk_start = i32(off_cblk), *line_start[2] = {i32(off_ls[0]), i32(off_ls[1])}, *line_face[2] = {i32(off_lf[0]), i32(off_lf[1])};
        uint64_t* crop_off = reinterpret_cast<uint64_t*>(head + off_cropoff);
        for (int f = 0; f < N; ++f) {
            const int32_t* g = geom + (size_t)f * kGeom;
            const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], pad = pad_of(f);
            const int Hp = Hr + 2 * pad, Wp = Wr + 2 * pad;
            const int top = std::max(0, pad - y0), left = std::max(0, pad - x0);
            const int bottom = std::max(0, y0 + Hr - 1 + pad - (Hs - 1)), right = std::max(0, x0 + Wr - 1 + pad - (Ws - 1));
            const int Hwin = Hp - top - bottom, Wwin = Wp - left - right;
            cblk_start[f] = (int32_t)cblks;
            crop_off[f] = bytes;
            cblks += cdiv((long)Hwin * Wwin, kCropPixels);
            bytes += ((uint64_t)Hp * Wp * 3 + 15) / 16 * 16;
            if (top || bottom) {   // axis 0: one line per column of the window
                line_face[0][nlf[0]] = f, line_start[0][nlf[0]++] = (int32_t)lines[0];
                lines[0] += Wwin;
            }
            if (left || right) {   // axis 1: one line per row of the crop, the rows axis 0 filled included
                line_face[1][nlf[1]] = f, line_start[1][nlf[1]++] = (int32_t)lines[1];
                lines[1] += Hp;
            }
        }
        cblk_start[N] = (int32_t)cblks;
        line_start[0][nlf[0]] = (int32_t)lines[0], line_start[1][nlf[1]] = (int32_t)lines[1];
    }
    bool fit_one_launch() const { return cblks <= INT32_MAX && lines[0] <= INT32_MAX && lines[1] <= INT32_MAX; }
    // ws: the workspace with the head in place, the crops from ws + off_crops; pads [N] on the device, or null and pad_all
    int launch(hipStream_t s, const unsigned char* src, const uint64_t* src_off, const int32_t* geom, const float* inv, unsigned char* ws,
               size_t off_crops, int N, const int32_t* pads, int pad_all) const {
        auto di32 = [&](size_t off) { return reinterpret_cast<const int32_t*>(ws + off); };
        const uint64_t* crop_off = reinterpret_cast<const uint64_t*>(ws + off_cropoff);
        hipLaunchKernelGGL(faces_crop_k, dim3((unsigned)cblks), dim3(256), 0, s, src, src_off, geom, inv, di32(off_cblk), crop_off, ws + off_crops, N,
                           pads, pad_all);
        CG_LAUNCH_CHECK();
        for (int axis = 0; axis < 2; ++axis) {
            if (!lines[axis]) continue;
            hipLaunchKernelGGL(faces_median_k, dim3((unsigned)lines[axis]), dim3(64), 0, s, geom, di32(off_lf[axis]), di32(off_ls[axis]), nlf[axis],
                               crop_off, ws + off_crops, pads, pad_all, axis);
            CG_LAUNCH_CHECK();
        }
        return 0;
    }
};

// The bands of rows of a horizontal pass and where each face's result lies in tmp: face f has hw(f) = (H, W) rows and columns going
// in, and per_row bytes of tmp per row
struct Bands {
    long bands = 0;
    uint64_t rows = 0;
    template <class HW>
    void plan(int32_t* band_start, uint64_t* tmp_off, int N, uint64_t per_row, const HW& hw) {
        for (int f = 0; f < N; ++f) {
            const auto [H, W] = hw(f);
            band_start[f] = (int32_t)bands;
            tmp_off[f] = rows * per_row;
            bands += cdiv(H, band_rows(W));
            rows += (uint64_t)H;
        }
        band_start[N] = (int32_t)bands;
    }
};
struct Side2 {
    int H, W;
};

// What the three entry points do alike around their own horizontal pass.  plan() brings the descriptors back, checks them and fills the
// workspace's head; upload() checks the workspace's size, puts the head in place and, where crops take part, enqueues them; vpass()
// enqueues the vertical pass.  The entry point says, in the order of the fields: per_face, the items of a face in tmp and dst; crops,
// whether the padded crops take part; padded, whether every face has a pad of its own, pads [N] on the device - then the bands, the
// ksizes and the tap tables belong to the padded sides, which pgeom holds - or all have pad_all.
// workspace: band_start [N + 1] int32 | with crops, Crops' maps: cblk_start [N + 1], the two median launches' line_start [N + 1] and
//            line_face [N] int32, crop_off [N] uint64 | tmp_off [N] uint64 | with padded, pgeom [N][8] int32, geom with the padded sides in
//            place of the rectangle's | with crops, the padded crops | tmp bytes
struct Job {
    const char* who;
    hipStream_t s;
    const unsigned char* src; const uint64_t* src_off; const int32_t* geom; const float* inv; const int32_t* taps; const uint64_t* tap_off;
    unsigned char* dst; int N, out; void* workspace; size_t workspace_bytes;
    int per_face; bool crops, padded; const int32_t* pads; int pad_all;
    Faces h;
    Crops c;
    Bands b;
    size_t off_band = 0, off_tmpoff = 0, off_pgeom = 0, off_crops = 0, off_tmp = 0;
    std::vector<unsigned char> head;
    unsigned char* ws = nullptr;   // the workspace once the head is in place
    int bpf = 0;                   // blocks per item of the vertical pass
    const int32_t* di32(size_t off) const { return reinterpret_cast<const int32_t*>(ws + off); }
    const uint64_t* du64(size_t off) const { return reinterpret_cast<const uint64_t*>(ws + off); }
    int plan(size_t src_bytes, size_t ntaps) {
        if (int rc = h.read(who, s, src, src_bytes, src_off, geom, inv, taps, ntaps, tap_off, dst, N, out, workspace, pads, padded)) return rc;
        Layout lay;
        off_band = lay.take((size_t)(N + 1) * 4);
        if (crops) c.reserve(lay, N);
        off_tmpoff = lay.take((size_t)N * 8);
        if (padded) off_pgeom = lay.take((size_t)N * kGeom * 4);
        off_crops = lay.bytes;
        head.assign(off_crops, 0);
        const int32_t* sides = h.geom.data();   // whose (H, W) go into the horizontal pass
        if (padded) {
            int32_t* pgeom = reinterpret_cast<int32_t*>(head.data() + off_pgeom);
            for (int f = 0; f < N; ++f) {
                std::copy_n(h.geom.data() + (size_t)f * kGeom, kGeom, pgeom + (size_t)f * kGeom);
                pgeom[(size_t)f * kGeom + 4] += 2 * h.pads[f], pgeom[(size_t)f * kGeom + 5] += 2 * h.pads[f];
            }
            sides = pgeom;
        }
        b.plan(reinterpret_cast<int32_t*>(head.data() + off_band), reinterpret_cast<uint64_t*>(head.data() + off_tmpoff), N,
               (uint64_t)per_face * out * 3, [&](int f) { return Side2{sides[(size_t)f * kGeom + 4], sides[(size_t)f * kGeom + 5]}; });
        if (crops) c.plan(head.data(), h.geom.data(), N, [&](int f) { return padded ? h.pads[f] : pad_all; });
        bpf = cdiv((long)out * out * 3, 256);
        off_tmp = off_crops + c.bytes;
        return 0;
    }
    bool fits_one_launch() const { return b.bands <= INT32_MAX && c.fit_one_launch() && (long)N * per_face * bpf <= INT32_MAX; }
    int upload() {
        const size_t need = off_tmp + b.rows * (size_t)per_face * out * 3;
        CG_REQUIRE(workspace_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed", who, workspace_bytes, need);
        ws = static_cast<unsigned char*>(workspace);
        CG_HIP(hipMemcpyAsync(ws, head.data(), head.size(), hipMemcpyHostToDevice, s));
        CG_HIP(hipStreamSynchronize(s));   // `head` is pageable and ends with this call
        return crops ? c.launch(s, src, src_off, geom, inv, ws, off_crops, N, pads, pad_all) : 0;
    }
    int vpass() const {
        hipLaunchKernelGGL(faces_vpass_k, dim3((unsigned)((long)N * per_face * bpf)), dim3(256), 0, s, ws + off_tmp, du64(off_tmpoff),
                           padded ? di32(off_pgeom) : geom, taps, tap_off, dst, out, bpf, per_face);
        CG_LAUNCH_CHECK();
        return 0;
    }
};

}  // namespace
}  // namespace cg

using namespace cg;

int cg_faces_u8_extract(void* stream, const unsigned char* src, size_t src_bytes, const uint64_t* src_off, const int32_t* geom,
                        const float* inv, const int32_t* taps, size_t ntaps, const uint64_t* tap_off, unsigned char* dst, int N, int out,
                        void* workspace, size_t workspace_bytes) {
    Job j{"cg_faces_u8_extract", S(stream), src, src_off, geom, inv, taps, tap_off, dst, N, out, workspace, workspace_bytes, 1, false, false, nullptr, 0};
    if (int rc = j.plan(src_bytes, ntaps)) return rc;
    CG_REQUIRE(j.fits_one_launch(), "%s: %ld bands of rows do not fit one launch", j.who, j.b.bands);
    if (int rc = j.upload()) return rc;
    hipLaunchKernelGGL(faces_warp_hpass_k, dim3((unsigned)j.b.bands), dim3(256), 0, j.s, src, src_off, geom, inv, taps, tap_off,
                       j.di32(j.off_band), j.du64(j.off_tmpoff), j.ws + j.off_tmp, N, out);
    CG_LAUNCH_CHECK();
    return j.vpass();
}

int cg_faces_u8_extract_variants(void* stream, const unsigned char* src, size_t src_bytes, const uint64_t* src_off, const int32_t* geom,
                                 const float* inv, const int32_t* taps, size_t ntaps, const uint64_t* tap_off, int pad, int A,
                                 const float* desc, const uint64_t* bases, float noise_scale, uint64_t seed, unsigned char* dst, int N, int out,
                                 void* workspace, size_t workspace_bytes) {
    static const char who[] = "cg_faces_u8_extract_variants";
    CG_REQUIRE(desc && bases, "%s: null pointer", who);
    CG_REQUIRE(pad >= 0 && pad <= 64, "%s: pad = %d is outside 0..64", who, pad);
    CG_REQUIRE(A >= 1 && A <= 999, "%s: A = %d is outside 1..999", who, A);
    CG_REQUIRE(noise_scale >= 0.f && noise_scale <= 3.0e38f, "%s: noise_scale = %g is negative or not finite", who, (double)noise_scale);
    Job j{who, S(stream), src, src_off, geom, inv, taps, tap_off, dst, N, out, workspace, workspace_bytes, A, true, false, nullptr, pad};
    if (int rc = j.plan(src_bytes, ntaps)) return rc;
    for (int f = 0; f < N; ++f) {
        const int Hp = j.h.geom[(size_t)f * kGeom + 4] + 2 * pad, Wp = j.h.geom[(size_t)f * kGeom + 5] + 2 * pad;
        CG_REQUIRE(Hp <= 4096 + 2 * 64 && Wp <= 4096 + 2 * 64, "%s: face %d: a padded crop of %d x %d is beyond %d", who, f, Wp, Hp, 4096 + 2 * 64);
    }
    CG_REQUIRE(j.fits_one_launch(), "%s: %d faces with %d variants (%ld bands of rows, %ld crop blocks) do not fit one launch", who, N, A,
               j.b.bands, j.c.cblks);
    if (int rc = j.upload()) return rc;
    hipLaunchKernelGGL(faces_variant_hpass_k, dim3((unsigned)j.b.bands, (unsigned)A), dim3(256), 0, j.s, j.ws + j.off_crops, j.du64(j.c.off_cropoff),
                       geom, desc, bases, taps, tap_off, j.di32(j.off_band), j.du64(j.off_tmpoff), j.ws + j.off_tmp, N, A, pad, out, noise_scale, seed);
    CG_LAUNCH_CHECK();
    return j.vpass();
}

int cg_faces_u8_extract_padded(void* stream, const unsigned char* src, size_t src_bytes, const uint64_t* src_off, const int32_t* geom,
                               const float* inv, const int32_t* taps, size_t ntaps, const uint64_t* tap_off, const int32_t* pads,
                               unsigned char* dst, int N, int out, void* workspace, size_t workspace_bytes) {
    Job j{"cg_faces_u8_extract_padded", S(stream), src, src_off, geom, inv, taps, tap_off, dst, N, out, workspace, workspace_bytes, 1, true, true, pads, 0};
    if (int rc = j.plan(src_bytes, ntaps)) return rc;
    CG_REQUIRE(j.fits_one_launch(), "%s: %d faces (%ld bands of rows, %ld crop blocks) do not fit one launch", j.who, N, j.b.bands, j.c.cblks);
    if (int rc = j.upload()) return rc;
    hipLaunchKernelGGL(faces_crop_hpass_k, dim3((unsigned)j.b.bands), dim3(256), 0, j.s, j.ws + j.off_crops, j.du64(j.c.off_cropoff),
                       j.di32(j.off_pgeom), taps, tap_off, j.di32(j.off_band), j.du64(j.off_tmpoff), j.ws + j.off_tmp, N, out);
    CG_LAUNCH_CHECK();
    return j.vpass();
}
