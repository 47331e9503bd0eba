// Nearest training-set neighbour search (sample.lua:131-151 on the device): squared 2-norm distances of up to 64 queries to every row
// of a pool chunk in the DIFFERENCE form, every operation a single fp32 one in an order that depends on D only (catgan.h,
// cg_nearest_update), the running best kept on the device.  No MFMA: ||t||^2 + ||q||^2 - 2 t.q cancels exactly where the answer
// matters (a near-duplicate), and no floating-point atomics: workgroups leave their candidates in the workspace, a finishing launch
// merges them under a total order.
#include "common.h"
#include <limits.h>

namespace cg {
namespace {

constexpr int kTile = 512;        // elements of one D tile = 64 lanes x 8 (part of the documented summation order)
constexpr int kPerLane = kTile / 64;
constexpr int kThreads = 512;     // 8 waves; each takes two rows at a time (one query read from the LDS serves both)
constexpr int kWaves = kThreads / 64;
constexpr int kMaxQ = 64;
constexpr int kMaxBlocks = 1024;  // workgroups of one launch = candidate rows of the workspace; more row blocks are walked grid-stride

// the sum of a row of 16 lanes as a butterfly: lane ^ 1, lane ^ 2, then the other quad pair, then the other half of the row.  After
// each step both partners hold the same value (a + b == b + a), so this is the binary tree over adjacent lanes
__device__ __forceinline__ float row16_sum(float s) {
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xf, 0xf, false));   // row_half_mirror
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x140, 0xf, 0xf, false));   // row_mirror
    return s;
}

#pragma clang fp contract(off)   // no fma: subtract, multiply, add are rounded one by one, as nn_utils.nearest_d2_np does
__global__ __launch_bounds__(kThreads) void nearest_rows_k(const float* __restrict__ pool, int N, long D, const float* __restrict__ queries,
                                                           int Q, int index0, int RB, int nrb, float* __restrict__ part_d,
                                                           int32_t* __restrict__ part_i) {
    extern __shared__ float nn_sh[];
    float* qs = nn_sh;                        // [Q][kTile]: the queries' slice of the current D tile, zero beyond D
    float* acc = nn_sh + (size_t)Q * kTile;   // [RB][64]: d2 of (row, query = lane) over the tiles done so far
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = (int)((D + kTile - 1) / kTile);
    const int groups = (Q + 3) >> 2;
    float best_d = __builtin_inff();
    int best_i = INT_MAX;
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const long row0 = (long)rb * RB;
        for (int i = tid; i < RB * 64; i += kThreads) acc[i] = 0.f;
        for (int t = 0; t < T; ++t) {
            const long e0 = (long)t * kTile;
            __syncthreads();   // the previous tile's readers are done
            for (int i = tid; i < Q * kTile; i += kThreads) {
                const long e = e0 + (i & (kTile - 1));
                qs[i] = e < D ? queries[(long)(i / kTile) * D + e] : 0.f;
            }
            __syncthreads();
            for (int pr = wave * 2; pr < RB; pr += 2 * kWaves) {
                // rows past the chunk's end are computed on the last row and dropped in the merge below
                const long na = std::min<long>(row0 + pr, N - 1), nb = std::min<long>(row0 + pr + 1, N - 1);
                const float* ra = pool + na * D + e0;
                const float* rbp = pool + nb * D + e0;
                float xa[kPerLane], xb[kPerLane];
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    const bool in = e0 + j * 64 + lane < D;
                    xa[j] = in ? ra[j * 64 + lane] : 0.f;
                    xb[j] = in ? rbp[j * 64 + lane] : 0.f;
                }
                float ta = 0.f, tb = 0.f;   // this tile's sums for query == lane
                for (int g = 0; g < groups; ++g) {
                    float va = 0.f, vb = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float* qv = qs + (size_t)std::min(4 * g + k, Q - 1) * kTile + lane;
                        float sa = 0.f, sb = 0.f;
#pragma unroll
                        for (int j = 0; j < kPerLane; ++j) {
                            const float q = qv[j * 64];
                            const float da = xa[j] - q, db = xb[j] - q;
                            sa = sa + da * da;
                            sb = sb + db * db;
                        }
                        sa = row16_sum(sa);
                        sb = row16_sum(sb);
                        va = (lane & 3) == k ? sa : va;
                        vb = (lane & 3) == k ? sb : vb;
                    }
                    // the last two levels of the tree for four queries at once: lane l carries query 4 g + (l & 3)
                    va = va + __shfl_xor(va, 16, 64);
                    vb = vb + __shfl_xor(vb, 16, 64);
                    va = va + __shfl_xor(va, 32, 64);
                    vb = vb + __shfl_xor(vb, 32, 64);
                    ta = (lane >> 2) == g ? va : ta;
                    tb = (lane >> 2) == g ? vb : tb;
                }
                acc[pr * 64 + lane] = acc[pr * 64 + lane] + ta;
                acc[(pr + 1) * 64 + lane] = acc[(pr + 1) * 64 + lane] + tb;
            }
        }
        __syncthreads();
        if (wave == 0) {   // rows in ascending order: the first of equal distances stays
            for (int r = 0; r < RB && row0 + r < N; ++r) {
                const float d = acc[r * 64 + lane];
                if (d < best_d) {
                    best_d = d;
                    best_i = index0 + (int)(row0 + r);
                }
            }
        }
        __syncthreads();   // before acc is cleared for the next row block
    }
    if (wave == 0) {
        part_d[blockIdx.x * 64 + lane] = best_d;
        part_i[blockIdx.x * 64 + lane] = best_i;
    }
}

__device__ __forceinline__ bool nearer(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// one workgroup of 256: four threads per query walk the candidate rows, thread q merges them into (best_d2, best_idx).  (d2, index) is a
// total order, so neither the split nor the order of the walk shows in the result
__global__ __launch_bounds__(256) void nearest_finish_k(const float* __restrict__ part_d, const int32_t* __restrict__ part_i, int nblocks, int Q,
                                                        int reset, float* __restrict__ best_d2, int32_t* __restrict__ best_idx) {
    __shared__ float sd[4][64];
    __shared__ int si[4][64];
    const int q = threadIdx.x & 63, s = threadIdx.x >> 6;
    float bd = __builtin_inff();
    int bi = INT_MAX;
    for (int b = s; b < nblocks; b += 4) {
        const float d = part_d[b * 64 + q];
        const int i = part_i[b * 64 + q];
        if (nearer(d, i, bd, bi)) { bd = d; bi = i; }
    }
    sd[s][q] = bd;
    si[s][q] = bi;
    __syncthreads();
    if (s == 0 && q < Q) {
        bd = reset ? __builtin_inff() : best_d2[q];
        bi = reset ? -1 : best_idx[q];
        for (int k = 0; k < 4; ++k)
            if (nearer(sd[k][q], si[k][q], bd, bi)) { bd = sd[k][q]; bi = si[k][q]; }
        best_d2[q] = bd;
        best_idx[q] = bi;
    }
}

// rows per workgroup (16 / 32 / 64: two per wave and pass) and the launch's workgroups: speed only, the sums do not depend on either
void nearest_geometry(int N, int& RB, int& nrb, int& blocks) {
    RB = N >= 32768 ? 64 : N >= 16384 ? 32 : 16;
    nrb = (N + RB - 1) / RB;
    blocks = std::min(nrb, kMaxBlocks);
}

}  // namespace
}  // namespace cg

extern "C" {

size_t cg_nearest_workspace_bytes(int N, int Q, long D) {
    (void)Q; (void)D;
    int RB, nrb, blocks;
    cg::nearest_geometry(std::max(N, 0), RB, nrb, blocks);
    return (size_t)std::max(blocks, 1) * 64 * (sizeof(float) + sizeof(int32_t));
}

int cg_nearest_update(void* stream, const float* pool, int N, long D, const float* queries, int Q, int index0, int reset, float* best_d2,
                      int32_t* best_idx, void* workspace) {
    using namespace cg;
    CG_REQUIRE(queries && best_d2 && best_idx && workspace && (pool || N == 0), "cg_nearest_update: null pointer");
    CG_REQUIRE(Q >= 1 && Q <= kMaxQ, "cg_nearest_update: Q = %d is outside 1..%d", Q, kMaxQ);
    CG_REQUIRE(N >= 0 && D >= 1, "cg_nearest_update: bad geometry N = %d, D = %ld", N, D);
    CG_REQUIRE(index0 >= 0 && (long)index0 + N <= (long)INT_MAX, "cg_nearest_update: index0 = %d with N = %d does not fit int32", index0, N);
    int RB = 0, nrb = 0, blocks = 0;
    nearest_geometry(N, RB, nrb, blocks);
    float* part_d = (float*)workspace;
    int32_t* part_i = (int32_t*)(part_d + (size_t)std::max(blocks, 1) * 64);
    if (N > 0) {
        // dynamic LDS: Q x 2 KB for the queries' slice of a tile + RB x 256 B for acc - up to 128 KB + 16 KB = 144 KB at Q = 64, RB = 64, which
        // relies on gfx950's 160 KB per workgroup (asked for once per thread and device; the hipGetDevice per call is what finds the device)
        const long lds = ((long)Q * kTile + (long)RB * 64) * sizeof(float);
        static thread_local int lds_dev = -1, lds_max = 0, lds_asked = 0;
        int dev = 0;
        CG_HIP(hipGetDevice(&dev));
        if (dev != lds_dev) {
            CG_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
            lds_dev = dev; lds_asked = 0;
        }
        CG_REQUIRE(lds <= lds_max, "cg_nearest_update: %d queries need %ld bytes of LDS, the device has %d per workgroup", Q, lds, lds_max);
        if (lds > 65536 && lds > lds_asked) {   // above 64 KB a kernel has to ask
            CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(nearest_rows_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
            lds_asked = lds_max;
        }
        hipLaunchKernelGGL(nearest_rows_k, dim3(blocks), dim3(kThreads), (size_t)lds, S(stream), pool, N, D, queries, Q, index0, RB, nrb, part_d,
                           part_i);
        CG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(nearest_finish_k, dim3(1), dim3(256), 0, S(stream), part_d, part_i, blocks, Q, reset, best_d2, best_idx);
    CG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
