// The validator network V and its trainer (models.lua:716-804, train_v.lua): nn.SoftMax on rows and the two device stages of the
// synthetic-fake generator (train_v.lua:294-668).  Descriptor layouts are documented in include/catgan.h.
#include "common.h"

namespace {

constexpr int kThreads = 256;

__device__ inline float seg_max(float v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float seg_sum(float v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide max / min of kThreads lanes through `red` (kThreads / 64 floats); every thread gets the result
__device__ float block_max(float v, float* red) {
    v = seg_max(v, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < kThreads / 64; ++i) r = fmaxf(r, red[i]);
    return r;
}
__device__ float block_min(float v, float* red) { return -block_max(-v, red); }

// ---------------------------------------------------------------------------------------------------------------- nn.SoftMax
// A row of n elements is handled by a segment of G = min(64, pow2 >= n) lanes of one wave (64 / G rows per wave); lane l of the segment
// holds elements l, l + G, ... in registers (R of them; R == 0: rows longer than 16 * 64, read again per pass).
template <int R>
__global__ void __launch_bounds__(kThreads) softmax_fwd_k(const float* __restrict__ x, float* __restrict__ y, long rows, int n, int G) {
    const int lane = threadIdx.x & 63, seg = lane / G, l = lane - seg * G;
    const long row = ((long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * (64 / G) + seg;
    const bool live = row < rows;
    const float* xr = x + (live ? row : 0) * n;
    float v[R > 0 ? R : 1];
    float mx = -INFINITY;
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < (R > 0 ? R : 1); ++k) {
            const int j = l + k * G;
            v[k] = (live && j < n) ? xr[j] : -INFINITY;
            mx = fmaxf(mx, v[k]);
        }
    } else if (live) {
        for (int j = l; j < n; j += G) mx = fmaxf(mx, xr[j]);
    }
    mx = seg_max(mx, G);
    float s = 0.f;
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < (R > 0 ? R : 1); ++k) {
            v[k] = (l + k * G < n) ? expf(v[k] - mx) : 0.f;
            s += v[k];
        }
    } else if (live) {
        for (int j = l; j < n; j += G) s += expf(xr[j] - mx);
    }
    s = seg_sum(s, G);
    if (!live) return;
    float* yr = y + row * n;
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < (R > 0 ? R : 1); ++k)
            if (l + k * G < n) yr[l + k * G] = v[k] / s;
    } else {
        for (int j = l; j < n; j += G) yr[j] = expf(xr[j] - mx) / s;
    }
}

// dx = y * (dy - sum_j dy_j y_j)
template <int R>
__global__ void __launch_bounds__(kThreads) softmax_bwd_k(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                          long rows, int n, int G) {
    const int lane = threadIdx.x & 63, seg = lane / G, l = lane - seg * G;
    const long row = ((long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * (64 / G) + seg;
    const bool live = row < rows;
    const long base = (live ? row : 0) * n;
    float yv[R > 0 ? R : 1], gv[R > 0 ? R : 1];
    float dot = 0.f;
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < (R > 0 ? R : 1); ++k) {
            const int j = l + k * G;
            const bool in = live && j < n;
            yv[k] = in ? y[base + j] : 0.f;
            gv[k] = in ? dy[base + j] : 0.f;
            dot += yv[k] * gv[k];
        }
    } else if (live) {
        for (int j = l; j < n; j += G) dot += y[base + j] * dy[base + j];
    }
    dot = seg_sum(dot, G);
    if (!live) return;
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < (R > 0 ? R : 1); ++k)
            if (l + k * G < n) dx[base + l + k * G] = yv[k] * (gv[k] - dot);
    } else {
        for (int j = l; j < n; j += G) dx[base + j] = y[base + j] * (dy[base + j] - dot);
    }
}

// ------------------------------------------------------------------------------------------------- synthetic-fake generator
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline int wrap(int v, int m) { v %= m; return v < 0 ? v + m : v; }   // withinImageCoords (train_v.lua:450-467), 0-based

// getGaussianOverlay(blur) (train_v.lua:533-561), one workgroup per overlay:
//   r = clamp(clamp(2 o1 - o2, 0, 1) + 2 o3 o4, 0, 1); blur > 0: r = image.convolve(r, image.gaussian(blur), "same") / max
// The composed overlay and the taps sit in LDS; the convolution accumulates in double.
__global__ void __launch_bounds__(kThreads) overlay_compose_k(const float* __restrict__ bank, int nbank, const int32_t* __restrict__ desc,
                                                              float* __restrict__ out, int H, int W) {
    extern __shared__ float lds[];
    __shared__ float taps[16 * 16];
    __shared__ float red[kThreads / 64];
    const int HW = H * W;
    float* r = lds;          // [HW] composed overlay
    float* c = lds + HW;     // [HW] blurred
    const int32_t* d = desc + blockIdx.x * 5;
    const float* o1 = bank + (long)clampi(d[0], 0, nbank - 1) * HW;
    const float* o2 = bank + (long)clampi(d[1], 0, nbank - 1) * HW;
    const float* o3 = bank + (long)clampi(d[2], 0, nbank - 1) * HW;
    const float* o4 = bank + (long)clampi(d[3], 0, nbank - 1) * HW;
    const int k = clampi(d[4], 0, 16);
    float* dst = out + (long)blockIdx.x * HW;
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        const float a = fminf(fmaxf(o1[p] * 2.f - o2[p], 0.f), 1.f);
        r[p] = fminf(fmaxf(a + (o3[p] * o4[p]) * 2.f, 0.f), 1.f);
    }
    if (k == 0) {
        __syncthreads();
        for (int p = threadIdx.x; p < HW; p += kThreads) dst[p] = r[p];
        return;
    }
    // image.gaussian(k): sigma 0.25, amplitude 1, unnormalised, centre 0.5 k + 0.5 (1-based taps), computed in double, stored as float
    for (int t = threadIdx.x; t < k * k; t += kThreads) {
        const int i = t / k + 1, j = t % k + 1;
        const double cen = 0.5 * k + 0.5, sw = 0.25 * k;
        const double u = (j - cen) / sw, v = (i - cen) / sw;
        taps[t] = (float)exp(-(u * u / 2.0 + v * v / 2.0));
    }
    __syncthreads();
    const int s = (k + 1) / 2 - 1;   // "same": rows / columns ceil(k/2) .. of the full convolution (1-based)
    float mx = -INFINITY;
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        const int y = p / W, x = p - y * W;
        double acc = 0.0;
        for (int u = 0; u < k; ++u) {
            const int yy = y + s - u;
            if (yy < 0 || yy >= H) continue;
            for (int v = 0; v < k; ++v) {
                const int xx = x + s - v;
                if (xx < 0 || xx >= W) continue;
                acc += (double)r[yy * W + xx] * (double)taps[u * k + v];
            }
        }
        c[p] = (float)acc;
        mx = fmaxf(mx, c[p]);
    }
    mx = block_max(mx, red);
    const float div = mx > 0.f ? mx : 1.f;   // an all-zero overlay stays zero (the reference would divide 0 by 0)
    for (int p = threadIdx.x; p < HW; p += kThreads) dst[p] = c[p] / div;
}

// y + (2 o - 1) len without contraction into FMAs: one rounding more or less moves a coordinate near the far border by an ulp of H
__device__ inline float warp_coord(int y, float o, float len) {
#pragma clang fp contract(off)
    return (float)y + (o * 2.f - 1.f) * len;
}

// One level of createSyntheticImages for one image into dst (LDS, the image's NHWC slice), normalised as the reference does.
__device__ void synth_level(const int32_t* d, const float* f, const float* __restrict__ pool, int npool, const float* __restrict__ ovl,
                            int novl, float* dst, float* red, int C, int H, int W) {
    const int HW = H * W, n = HW * C;
    const int kind = d[0];
    const float* A = pool + (long)clampi(d[1], 0, npool - 1) * n;
    const float* B = pool + (long)clampi(d[2], 0, npool - 1) * n;
    const float* OA = ovl + (long)clampi(d[3], 0, novl - 1) * HW;
    const float* OB = ovl + (long)clampi(d[4], 0, novl - 1) * HW;
    const float* OC = ovl + (long)clampi(d[5], 0, novl - 1) * HW;
    const int p0 = d[6], p1 = d[7];
    float mx = -INFINITY, mn = INFINITY;
    for (int e = threadIdx.x; e < n; e += kThreads) {
        const int p = e / C, c = e - p * C, y = p / W, x = p - y * W;
        float v;
        if (kind == 0) {            // Mix (:327-382): o a + (1 - o) b
            const float o = OA[p];
            v = o * A[e] + (1.f - o) * B[e];
        } else if (kind == 1) {     // Stamp (:388-444): (1 - o) a[y,x] + o a[wrap(y + dy, x + dx)]
            const int q = wrap(y + p0, H) * W + wrap(x + p1, W);
            const float o = OA[p];
            v = (1.f - o) * A[e] + o * A[q * C + c];
        } else if (kind == 2) {     // Warp (:450-484): image.warp(a, flow), flow = (2 o - 1) * length, bilinear, offset mode, clamped
            const float len = f[0];
            float iy = warp_coord(y, OA[p], len), ix = warp_coord(x, OB[p], len);
            iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
            ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
            const int y0 = (int)floorf(iy), x0 = (int)floorf(ix);
            const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
            const float wy = iy - (float)y0, wx = ix - (float)x0;
            const float top = (1.f - wx) * A[(y0 * W + x0) * C + c] + wx * A[(y0 * W + x1) * C + c];
            const float bot = (1.f - wx) * A[(y1 * W + x0) * C + c] + wx * A[(y1 * W + x1) * C + c];
            v = (1.f - wy) * top + wy * bot;
        } else {                    // Random (:490-528): base[c] + o1[y,x] o2[q] - o3[q], q = wrap(y + (c+1) offY, x + (c+1) offX)
            const int q = wrap(y + (c + 1) * p0, H) * W + wrap(x + (c + 1) * p1, W);
            v = f[c] + OA[p] * OB[q] - OC[q];
        }
        dst[e] = v;
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
    }
    mx = block_max(mx, red);
    float add = 0.f;
    if (kind == 3) {                // img:add(math.abs(torch.min(img))) - the absolute value even when the minimum is positive
        add = fabsf(block_min(mn, red));
        mx = mx + add;              // rounding is monotone: max(v + add) == max(v) + add
    }
    for (int e = threadIdx.x; e < n; e += kThreads) dst[e] = (dst[e] + add) / mx;
    __syncthreads();
}

// One workgroup per output image: level 1 (and the optional level 2 plus their mix, :309-313,350-365) in LDS, result to dst (NHWC).
__global__ void __launch_bounds__(kThreads) synth_images_k(const float* __restrict__ pool, int npool, const float* __restrict__ ovl, int novl,
                                                           const int32_t* __restrict__ idesc, const float* __restrict__ fdesc,
                                                           float* __restrict__ out, int C, int H, int W) {
    extern __shared__ float lds[];
    __shared__ float red[kThreads / 64];
    const int HW = H * W, n = HW * C;
    float* LA = lds;
    float* LB = lds + n;
    const int32_t* d = idesc + blockIdx.x * 18;
    const float* f = fdesc + blockIdx.x * 8;
    float* dst = out + (long)blockIdx.x * n;
    synth_level(d, f, pool, npool, ovl, novl, LA, red, C, H, W);
    if (d[8] < 0) {
        for (int e = threadIdx.x; e < n; e += kThreads) dst[e] = LA[e];
        return;
    }
    synth_level(d + 8, f + 4, pool, npool, ovl, novl, LB, red, C, H, W);
    const float* O = ovl + (long)clampi(d[16], 0, novl - 1) * HW;
    float mx = -INFINITY;
    for (int e = threadIdx.x; e < n; e += kThreads) {
        const float o = O[e / C];
        const float v = o * LA[e] + (1.f - o) * LB[e];
        LA[e] = v;
        mx = fmaxf(mx, v);
    }
    mx = block_max(mx, red);
    for (int e = threadIdx.x; e < n; e += kThreads) dst[e] = LA[e] / mx;
}

template <int R>
int softmax_launch(bool fwd, void* stream, const float* a, const float* b, float* out, long rows, int n, int G) {
    const long rows_per_block = (long)(kThreads / 64) * (64 / G);
    const dim3 grid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
    if (fwd)
        hipLaunchKernelGGL(softmax_fwd_k<R>, grid, dim3(kThreads), 0, cg::S(stream), a, out, rows, n, G);
    else
        hipLaunchKernelGGL(softmax_bwd_k<R>, grid, dim3(kThreads), 0, cg::S(stream), a, b, out, rows, n, G);
    CG_LAUNCH_CHECK();
    return 0;
}

int softmax_dispatch(bool fwd, void* stream, const float* a, const float* b, float* out, long rows, int n) {
    int G = 1;
    while (G < n && G < 64) G <<= 1;
    const int per = (n + G - 1) / G;
    if (per <= 1) return softmax_launch<1>(fwd, stream, a, b, out, rows, n, G);
    if (per <= 2) return softmax_launch<2>(fwd, stream, a, b, out, rows, n, G);
    if (per <= 4) return softmax_launch<4>(fwd, stream, a, b, out, rows, n, G);
    if (per <= 8) return softmax_launch<8>(fwd, stream, a, b, out, rows, n, G);
    if (per <= 16) return softmax_launch<16>(fwd, stream, a, b, out, rows, n, G);
    return softmax_launch<0>(fwd, stream, a, b, out, rows, n, G);
}

constexpr size_t kMaxLds = 160 * 1024 - 4096;   // gfx950: 160 KB per CU, less the static reduction / tap arrays

}  // namespace

extern "C" {

int cg_softmax_forward(void* stream, const float* x, float* y, long rows, int n) {
    CG_REQUIRE(x && y, "cg_softmax_forward: null pointer");
    CG_REQUIRE(rows >= 0 && n > 0, "cg_softmax_forward: bad geometry rows=%ld n=%d", rows, n);
    if (rows == 0) return 0;
    return softmax_dispatch(true, stream, x, nullptr, y, rows, n);
}

int cg_softmax_backward(void* stream, const float* y, const float* dy, float* dx, long rows, int n) {
    CG_REQUIRE(y && dy && dx, "cg_softmax_backward: null pointer");
    CG_REQUIRE(rows >= 0 && n > 0, "cg_softmax_backward: bad geometry rows=%ld n=%d", rows, n);
    if (rows == 0) return 0;
    return softmax_dispatch(false, stream, y, dy, dx, rows, n);
}

int cg_synth_overlays(void* stream, const float* bank, int nbank, const int32_t* desc, float* out, int count, int H, int W) {
    CG_REQUIRE(bank && desc && out, "cg_synth_overlays: null pointer");
    CG_REQUIRE(nbank > 0 && count >= 0 && H > 0 && W > 0, "cg_synth_overlays: bad geometry nbank=%d count=%d H=%d W=%d", nbank, count, H, W);
    const size_t lds = 2 * (size_t)H * W * sizeof(float);
    CG_REQUIRE(lds <= kMaxLds, "cg_synth_overlays: bad geometry (%dx%d overlays do not fit in LDS)", H, W);
    if (count == 0) return 0;
    static bool granted = false;
    if (lds > 64 * 1024 && !granted) {
        CG_HIP(hipFuncSetAttribute((const void*)overlay_compose_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
        granted = true;
    }
    hipLaunchKernelGGL(overlay_compose_k, dim3(count), dim3(kThreads), lds, cg::S(stream), bank, nbank, desc, out, H, W);
    CG_LAUNCH_CHECK();
    return 0;
}

int cg_synth_images(void* stream, const float* pool, int npool, const float* overlays, int noverlays, const int32_t* idesc,
                    const float* fdesc, float* dst, int count, int C, int H, int W) {
    CG_REQUIRE(pool && overlays && idesc && fdesc && dst, "cg_synth_images: null pointer");
    CG_REQUIRE(npool > 0 && noverlays > 0 && count >= 0 && C > 0 && C <= 4 && H > 0 && W > 0,
               "cg_synth_images: bad geometry npool=%d noverlays=%d count=%d C=%d H=%d W=%d", npool, noverlays, count, C, H, W);
    const size_t lds = 2 * (size_t)C * H * W * sizeof(float);
    CG_REQUIRE(lds <= kMaxLds, "cg_synth_images: bad geometry (%dx%dx%d images do not fit in LDS)", C, H, W);
    if (count == 0) return 0;
    static bool granted = false;
    if (lds > 64 * 1024 && !granted) {
        CG_HIP(hipFuncSetAttribute((const void*)synth_images_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
        granted = true;
    }
    hipLaunchKernelGGL(synth_images_k, dim3(count), dim3(kThreads), lds, cg::S(stream), pool, npool, overlays, noverlays, idesc, fdesc,
                       dst, C, H, W);
    CG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
