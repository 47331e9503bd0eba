// nn.MSECriterion (pretrain_g.lua:101,168-172), sizeAverage: *loss = (1/n) sum (x - t)^2, dx = (2/n) (x - t).
//
// The forward is a bandwidth-bound reduction over a whole image batch (49 152 elements at the script's batch of 16, 1.5 M at
// 128 x 3 x 64 x 64) whose ORDER is a function of n alone - not of the launch, not of the pointers' alignment:
//   * the elements are cut into chunks of kChunk = 4096.  Within a chunk, thread t of 256 owns the quads q = j * 256 + t, j = 0..3
//     (elements 4 q .. 4 q + 3) and adds their squares to its fp64 accumulator in the order j, then x y z w;
//   * P = min(ceil(n / kChunk), kMaxPartials) workgroups; workgroup p walks the chunks p, p + P, p + 2 P, ... with the same 256
//     accumulators, then sums them: 64 lanes as a shuffle tree (offsets 32, 16, .., 1), the four waves as ((w0 + w1) + w2) + w3;
//   * the P partials go to the stream's reduction scratch; the LAST workgroup to arrive (cg::last_block_arrives: a ticket, no
//     floating-point atomics) adds them - thread t takes p = t, t + 256, ..., then the same block sum - and writes
//     (float)(sum / n).  Which workgroup does that depends on timing, the order of the additions does not.
// x - t is one fp32 subtraction, as Torch7's THNN does; its square is exact in fp64 (24 + 24 bits) and every sum is fp64, so the
// result is the correctly rounded fp32 value or its neighbour (relative error of the sum <= n 2^-53).
// The aligned path (n % 4 == 0, both pointers 16-byte aligned) reads a quad as one 16-byte load, the other path as four scalar
// loads with an element guard: the same elements in the same accumulators, hence the same bits.
//
// nn.BCECriterion, the adversarial loss, follows the MSE kernels: one workgroup sums a batch of sigmoid outputs in fp64.
#include "common.h"

namespace cg {
namespace {

constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 4;                          // j = 0..3
constexpr long kChunk = 4L * kThreads * kQuadsPerThread;    // 4096 elements: part of the documented summation order
constexpr int kMaxPartials = 1024;                          // workgroups of one launch; more chunks are walked with stride P

__device__ __forceinline__ double sq(float a, float b) {
    const float d = a - b;
    return (double)d * (double)d;
}

template <bool V4>
__global__ __launch_bounds__(kThreads) void mse_fwd_k(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ loss,
                                                      long n, long nchunks, unsigned* counter, double* part) {
    __shared__ double sh[4];
    const int P = gridDim.x;
    double acc = 0.0;
    for (long c = blockIdx.x; c < nchunks; c += P) {
        const long q0 = c * (kChunk / 4);
#pragma unroll
        for (int j = 0; j < kQuadsPerThread; ++j) {
            const long e = 4 * (q0 + j * kThreads + threadIdx.x);
            if (V4) {
                if (e < n) {   // n % 4 == 0: the quad is whole
                    const float4 a = *reinterpret_cast<const float4*>(x + e), b = *reinterpret_cast<const float4*>(t + e);
                    acc += sq(a.x, b.x);
                    acc += sq(a.y, b.y);
                    acc += sq(a.z, b.z);
                    acc += sq(a.w, b.w);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < n) acc += sq(x[e + k], t[e + k]);
            }
        }
    }
    const double tot = block_sum_256(acc, sh);
    if (P == 1) {
        if (threadIdx.x == 0) *loss = (float)(tot / (double)n);
        return;
    }
    if (threadIdx.x == 0) st_agent(&part[blockIdx.x], tot);
    if (!last_block_arrives(counter, (unsigned)P)) return;
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += kThreads) s += ld_agent(&part[p]);
    const double all = block_sum_256(s, sh);
    if (threadIdx.x == 0) *loss = (float)(all / (double)n);
}

template <bool V4>
__global__ __launch_bounds__(kThreads) void mse_bwd_k(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ dx, long n) {
    const float norm = 2.f / (float)n;
    const long m = V4 ? n / 4 : n;
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < m; i += (long)gridDim.x * kThreads) {
        if (V4) {
            const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(t)[i];
            reinterpret_cast<float4*>(dx)[i] = make_float4(norm * (a.x - b.x), norm * (a.y - b.y), norm * (a.z - b.z), norm * (a.w - b.w));
        } else {
            dx[i] = norm * (x[i] - t[i]);
        }
    }
}

// ------------------------------------------------------------------------ BCE
__global__ void bce_fwd_k(const float* p, const float* t, float* loss, long n) {
    // single block: n is the batch size
    __shared__ double sh[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const float x = p[i], y = t[i];
        s -= (double)(logf(x + 1e-12f) * y + logf(1.f - x + 1e-12f) * (1.f - y));
    }
    const double tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) *loss = (float)(tot / (double)n);
}
__global__ void bce_bwd_k(const float* p, const float* t, float* dp, long n) {
    const float norm = 1.f / (float)n;
    CG_GRID_STRIDE(i, n) {
        const float x = p[i], y = t[i];
        dp[i] = -norm * (y - x) / ((1.f - x + 1e-12f) * (x + 1e-12f));
    }
}

}  // namespace
}  // namespace cg

extern "C" {

int cg_bce_forward(void* stream, const float* p, const float* t, float* loss, long n) {
    CG_REQUIRE(p && t && loss && n > 0, "cg_bce_forward: bad args");
    hipLaunchKernelGGL(cg::bce_fwd_k, dim3(1), dim3(256), 0, cg::S(stream), p, t, loss, n);
    CG_LAUNCH_CHECK(); return 0;
}
int cg_bce_backward(void* stream, const float* p, const float* t, float* dp, long n) {
    CG_REQUIRE(p && t && dp, "cg_bce_backward: null pointer");
    CG_EW_LAUNCH(cg::bce_bwd_k, n, p, t, dp, n); return 0;
}

int cg_mse_forward(void* stream, const float* x, const float* t, float* loss, long n) {
    using namespace cg;
    CG_REQUIRE(x && t && loss, "cg_mse_forward: null pointer");
    CG_REQUIRE(n > 0, "cg_mse_forward: bad length n = %ld", n);
    const long nchunks = (n + kChunk - 1) / kChunk;
    const int P = (int)std::min<long>(nchunks, kMaxPartials);
    unsigned* counter = nullptr;
    double* part = nullptr;
    if (P > 1) {   // ticket at the front of the stream's reduction scratch (zero between launches), partials behind it
        char* scr = (char*)col_scratch(S(stream));
        if (!scr) return 1;
        counter = (unsigned*)scr;
        part = (double*)(scr + 256);
        static_assert(256 + sizeof(double) * kMaxPartials <= kColScratchBytes, "partials exceed the scratch");
    }
    if (vec_ok(n, x, t))
        hipLaunchKernelGGL(mse_fwd_k<true>, dim3(P), dim3(kThreads), 0, S(stream), x, t, loss, n, nchunks, counter, part);
    else
        hipLaunchKernelGGL(mse_fwd_k<false>, dim3(P), dim3(kThreads), 0, S(stream), x, t, loss, n, nchunks, counter, part);
    CG_LAUNCH_CHECK();
    return 0;
}

int cg_mse_backward(void* stream, const float* x, const float* t, float* dx, long n) {
    using namespace cg;
    CG_REQUIRE(x && t && dx, "cg_mse_backward: null pointer");
    CG_REQUIRE(n > 0, "cg_mse_backward: bad length n = %ld", n);
    CG_EW_LAUNCH_V(vec_ok(n, x, t, dx), mse_bwd_k<V == 4>, n, x, t, dx, n);   // blocks of 256 = kThreads
    return 0;
}

}  // extern "C"
