// Differentiable augmentation of D's input (train.py --D_diffaug; Zhao et al. 2020; not in the reference): cg_diffaug_forward and its
// adjoint cg_diffaug_backward, catgan.h.  One workgroup of 1024 lanes per image (16 waves: the passes below are bound by latency, not by
// bandwidth), the image staged in the LDS as fp32 [H][W][C], so the whole transform is one read of x and one write of y whatever the
// policy:
//   stage   global -> LDS, 16 bytes per lane (the scalar twin: 4), raw bits.  Every global read of the image happens here, in front of
//           the first barrier, and every global write behind the last one: y == x is safe and gives the out-of-place bits
//   pixel   forward: brightness and saturation in place, one lane per pixel, and the image's fp64 sum for the contrast mean
//           backward: zero what the cutout covered and what the translation moved out of the image (in place, in gy's coordinates),
//           and the fp64 sum of the rest, which is the sum of the translated gradient
//   output  one lane per 4 (1) output floats: the cutout test, the translated LDS read, the contrast (forward) or the contrast and the
//           saturation of the source pixel (backward)
// The fp64 sums run over the LDS copy in a fixed order (lane-strided, then the waves in turn): the same bits for every N, every position
// of the image in the batch and either twin.  Nothing is added atomically.
#include "common.h"

namespace {
using cg::Vec;

constexpr int kColor = 1, kTranslation = 2, kCutout = 4;
constexpr long kMaxImageBytes = 65536;
constexpr int kLanes = 1024, kWaves = kLanes / 64;

__host__ __device__ __forceinline__ int round_of(int L, float f) { return (int)((float)L * f + 0.5f); }

// contrast around the image's mean and saturation around the pixel's mean, forward and adjoint alike (both operators are symmetric):
// (v - m) k + m, the difference rounded, then one fma
__device__ __forceinline__ float mix(float v, float m, float k) { return fmaf(v - m, k, m); }
template <int C>
__device__ __forceinline__ void saturate(float (&v)[C], float s) {
    if constexpr (C == 3) {
        const float m = ((v[0] + v[1]) + v[2]) / 3.f;
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = mix(v[k], m, s);
    }
}

struct Draw {
    float b, s, c;
    int tx, ty, r0, c0, ch, cw;   // the shift; the cutout's first row / column and its size
};

// an integer field of a descriptor the host placed by hand (draw == 0): anything, NaN included, lands inside [lo, hi], beyond which
// nothing of the image is reached any more
__device__ __forceinline__ int field(float v, int lo, int hi) { return (int)fminf(fmaxf(v, (float)lo), (float)hi); }

// image n's descriptor: lane 0 draws it (counters ctr .. ctr + 6; ctr + 7 is reserved) and stores it, or reads it; every lane gets it
__device__ __forceinline__ Draw descriptor(float* sd, float* dn, bool draw, uint64_t seed, uint64_t ctr, int H, int W, int policy) {
    const int ch = round_of(H, 0.5f), cw = round_of(W, 0.5f);
    if (threadIdx.x == 0) {
        if (draw) {
            const int Rw = round_of(W, 0.125f), Rh = round_of(H, 0.125f);
            float u[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) u[k] = cg::u01(seed, ctr + k);
            sd[0] = u[0] - 0.5f;
            sd[1] = 2.f * u[1];
            sd[2] = u[2] + 0.5f;
            sd[3] = floorf(u[3] * (float)(2 * Rw + 1)) - (float)Rw;
            sd[4] = floorf(u[4] * (float)(2 * Rh + 1)) - (float)Rh;
            sd[5] = floorf(u[5] * (float)(H + 1 - ch % 2));
            sd[6] = floorf(u[6] * (float)(W + 1 - cw % 2));
            sd[7] = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) dn[k] = sd[k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) sd[k] = dn[k];
        }
    }
    __syncthreads();
    Draw d;
    d.b = sd[0]; d.s = sd[1]; d.c = sd[2];
    d.tx = (policy & kTranslation) ? field(sd[3], -W, W) : 0;
    d.ty = (policy & kTranslation) ? field(sd[4], -H, H) : 0;
    d.ch = ch; d.cw = cw;
    d.r0 = field(sd[5], -H, 2 * H) - ch / 2;
    d.c0 = field(sd[6], -W, 2 * W) - cw / 2;
    return d;
}
__device__ __forceinline__ bool in_cutout(const Draw& d, int policy, int y, int x) {
    return (policy & kCutout) && y >= d.r0 && y < d.r0 + d.ch && x >= d.c0 && x < d.c0 + d.cw;
}
__device__ __forceinline__ bool in_image(int y, int x, int H, int W) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; }

// the block's fp64 sum - each wave's, then the waves' in turn - as the image's fp32 mean, in every lane
__device__ __forceinline__ float block_mean(double acc, int L, double* sh /*[kWaves]*/, float* sm) {
    acc = cg::wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += sh[w];
        *sm = (float)(t / (double)L);
    }
    __syncthreads();
    return *sm;
}

template <int VW>
__device__ __forceinline__ void stage(float* img, const float* src, int L) {
    for (int i = threadIdx.x; i < L / VW; i += kLanes) Vec<VW>::st(img + VW * i, Vec<VW>::ld(src + VW * i));
}

template <int C, int VW>
__global__ __launch_bounds__(kLanes) void diffaug_fwd_k(const float* x, float* y, float* desc, int H, int W, int policy, int draw,
                                                     uint64_t seed, uint64_t offset, const uint64_t* base) {
    extern __shared__ __align__(16) float img[];
    __shared__ float sd[8];
    __shared__ double sh[kWaves];
    __shared__ float sm;
    const int n = blockIdx.x, L = H * W * C;
    stage<VW>(img, x + (long)n * L, L);
    const Draw d = descriptor(sd, desc + (long)n * 8, draw != 0, seed, offset + (base ? *base : 0ull) + 8ull * n, H, W, policy);   // its barrier ends the stage
    float M = 0.f;
    if (policy & kColor) {
        double acc = 0.0;
        for (int p = threadIdx.x; p < H * W; p += kLanes) {
            float v[C];
#pragma unroll
            for (int k = 0; k < C; ++k) v[k] = img[p * C + k] + d.b;
            saturate<C>(v, d.s);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                img[p * C + k] = v[k];
                acc += (double)v[k];
            }
        }
        M = block_mean(acc, L, sh, &sm);
    }
    float* yn = y + (long)n * L;
    for (int i = threadIdx.x; i < L / VW; i += kLanes) {
        Vec<VW> o;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const int e = VW * i + k, pix = e / C, c = e - pix * C, yy = pix / W, xx = pix - yy * W;
            const int ys = yy - d.ty, xs = xx - d.tx;
            float v = 0.f;
            if (!in_cutout(d, policy, yy, xx) && in_image(ys, xs, H, W)) {
                v = img[(ys * W + xs) * C + c];
                if (policy & kColor) v = mix(v, M, d.c);
            }
            o[k] = v;
        }
        o.store(yn, i);
    }
}

template <int C, int VW>
__global__ __launch_bounds__(kLanes) void diffaug_bwd_k(const float* gy, float* gx, const float* desc, int H, int W, int policy) {
    extern __shared__ __align__(16) float img[];
    __shared__ float sd[8];
    __shared__ double sh[kWaves];
    __shared__ float sm;
    const int n = blockIdx.x, L = H * W * C;
    stage<VW>(img, gy + (long)n * L, L);
    const Draw d = descriptor(sd, const_cast<float*>(desc) + (long)n * 8, false, 0, 0, H, W, policy);
    // gy[Y][X] reaches gx[Y - ty][X - tx], unless the cutout covered (Y, X) or that lies outside the image
    double acc = 0.0;
    for (int e = threadIdx.x; e < L; e += kLanes) {
        const int pix = e / C, yy = pix / W, xx = pix - yy * W;
        if (in_cutout(d, policy, yy, xx) || !in_image(yy - d.ty, xx - d.tx, H, W)) img[e] = 0.f;
        else acc += (double)img[e];
    }
    float Gm = 0.f;
    if (policy & kColor) Gm = block_mean(acc, L, sh, &sm);
    else __syncthreads();
    float* gn = gx + (long)n * L;
    for (int i = threadIdx.x; i < L / VW; i += kLanes) {
        Vec<VW> o;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const int e = VW * i + k, pix = e / C, c = e - pix * C, yy = pix / W, xx = pix - yy * W;
            const int ys = yy + d.ty, xs = xx + d.tx;
            const bool in = in_image(ys, xs, H, W);
            float v[C];
#pragma unroll
            for (int j = 0; j < C; ++j) v[j] = in ? img[(ys * W + xs) * C + j] : 0.f;
            if (policy & kColor) {
#pragma unroll
                for (int j = 0; j < C; ++j) v[j] = mix(v[j], Gm, d.c);
                saturate<C>(v, d.s);
            }
            float r = v[0];
#pragma unroll
            for (int j = 1; j < C; ++j) r = c == j ? v[j] : r;
            o[k] = r;
        }
        o.store(gn, i);
    }
}

// what both entry points refuse, all of it before any HIP call
int check(const char* who, const void* a, const void* b, const void* desc, int N, int H, int W, int C, int policy) {
    CG_REQUIRE(a && b && desc, "%s: null pointer", who);
    CG_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad geometry (N = %d, H = %d, W = %d)", who, N, H, W);
    CG_REQUIRE(C == 1 || C == 3, "%s: C = %d, an image has 1 or 3 channels", who, C);
    CG_REQUIRE(policy >= 1 && policy <= 7, "%s: policy %d outside 1..7 (1 colour, 2 translation, 4 cutout)", who, policy);
    const long lds = (long)H * W * C * (long)sizeof(float);
    CG_REQUIRE(lds <= kMaxImageBytes, "%s: a %d x %d x %d image needs %ld bytes of LDS, a workgroup stages at most %ld", who, W, H, C, lds,
               kMaxImageBytes);
    return 0;
}
// the image in dynamic LDS beside the kernels' few static words: at the very top of the 64 KB the kernel has to ask
template <class K>
int lds_for(K kern, long lds) {
    if (lds + 256 > 65536) CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}
#define DIFFAUG_LAUNCH(kern, ...)                                                                       \
    do {                                                                                                \
        if (lds_for(kern, lds)) return 1;                                                               \
        hipLaunchKernelGGL(kern, dim3(N), dim3(kLanes), (size_t)lds, cg::S(stream), __VA_ARGS__);          \
        CG_LAUNCH_CHECK();                                                                              \
    } while (0)
// the float4-or-scalar twins of either channel count
#define DIFFAUG_DISPATCH(kern, ...)                                                                     \
    do {                                                                                                \
        if (C == 3) { if (vec) DIFFAUG_LAUNCH((kern<3, 4>), __VA_ARGS__); else DIFFAUG_LAUNCH((kern<3, 1>), __VA_ARGS__); } \
        else { if (vec) DIFFAUG_LAUNCH((kern<1, 4>), __VA_ARGS__); else DIFFAUG_LAUNCH((kern<1, 1>), __VA_ARGS__); }        \
    } while (0)
}  // namespace

extern "C" {

int cg_diffaug_forward(void* stream, const float* x, float* y, float* desc, int N, int H, int W, int C, int policy, int draw, uint64_t seed,
                       uint64_t offset, const uint64_t* base) {
    if (check("cg_diffaug_forward", x, y, desc, N, H, W, C, policy)) return 1;
    const long L = (long)H * W * C, lds = L * (long)sizeof(float);
    const bool vec = cg::vec_ok(L, x, y);
    DIFFAUG_DISPATCH(diffaug_fwd_k, x, y, desc, H, W, policy, draw, seed, offset, base);
    return 0;
}

int cg_diffaug_backward(void* stream, const float* gy, float* gx, const float* desc, int N, int H, int W, int C, int policy) {
    if (check("cg_diffaug_backward", gy, gx, desc, N, H, W, C, policy)) return 1;
    const long L = (long)H * W * C, lds = L * (long)sizeof(float);
    const bool vec = cg::vec_ok(L, gy, gx);
    DIFFAUG_DISPATCH(diffaug_bwd_k, gy, gx, desc, H, W, policy);
    return 0;
}

}  // extern "C"
