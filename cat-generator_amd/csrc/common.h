// Shared helpers for the gfx950 kernels behind include/catgan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/catgan.h"

namespace cg {

// thread-local error string returned by cg_last_error()
char* err_buf();
int fail(const char* fmt, ...);

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define CG_HIP(call)                                                              \
    do {                                                                          \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess)                                                    \
            return cg::fail("%s:%d %s -> %s", __FILE__, __LINE__, #call,          \
                            hipGetErrorString(e__));                              \
    } while (0)

#define CG_LAUNCH_CHECK()                                                         \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess)                                                    \
            return cg::fail("%s:%d kernel launch -> %s", __FILE__, __LINE__,      \
                            hipGetErrorString(e__));                              \
    } while (0)

#define CG_REQUIRE(cond, ...)                                                     \
    do {                                                                          \
        if (!(cond)) return cg::fail(__VA_ARGS__);                                \
    } while (0)

constexpr int kNumCU = 256;  // MI355X: 8 XCDs x 32 CUs

// Timing-only builds (VERDICT r05 #6e: the sensitivity numbers that steer the work must be reproducible from the repo).
//   CG_BUILD_DEFINES="-DCG_TIMING_PROBE=<mask>" python -c "import __graft_entry__ as g; g.build()"
// makes every K loop of the masked GEMM families run HALF its tiles - the same launches, the same memory-bound kernels around them,
// wrong results by construction - so that `python bench.py` shows how much of a family's duration the step's time follows:
//   1 direct implicit GEMMs (igemm_nn / igemm_nng)   2 weight gradients (igemm_tn / igemm_tng)   4 Winograd GEMMs (wino_gemm / wino_gemm_g)
//   8 the fused Winograd kernel's position loops (wino3_fused_k)
// Never set in a build whose results are used; cg_abi_version() of such a build returns -1 so that every host refuses it.
#ifndef CG_TIMING_PROBE
#define CG_TIMING_PROBE 0
#endif
#define CG_PROBE_HALF(fam, T) (((CG_TIMING_PROBE) & (fam)) ? ((T) + 1) / 2 : (T))
// grid caps of the memory-bound kernels, swept in round 4 and constants since round 6 (profiles/r04_sweeps.txt): 4 workgroups per CU for the
// grid-stride kernels (8 until round 4: beside another queue's GEMM fewer, longer-lived workgroups get through sooner), 1 per CU for the
// column reductions
constexpr int kEwWgsPerCU = 4, kColReduceWgsPerCU = 1;

// Tunables (cg_set_option / cg_get_option, catgan.h).  Default = the environment variable of the same name if set,
// else the built-in value; cg_set_option overrides both at run time (tests force every kernel variant this way).
enum Opt {
    OPT_SKINNY, OPT_GEMM_BK32, OPT_WINO_BK, OPT_NN_TILE, OPT_TN_TILE, OPT_NN_SPLITS, OPT_TN_SPLITS,
    OPT_XCD_SWIZZLE, OPT_NN_GLDS, OPT_TN_GLDS, OPT_WINO_GLDS, OPT_PAD_SKIP, OPT_WINO3, OPT_WINO_DGRAD_FUSE, OPT_WINO_DGRAD_FUSE_LAUNCHES,
    OPT_WINO3_LAUNCHES, OPT_PACK_WIDE, OPT_SAMPLER_ATOMIC_LAUNCHES, OPT_COUNT
};
long opt(Opt o);
// CG_WINO_DGRAD_FUSE_LAUNCHES and CG_WINO3_LAUNCHES are not tunables but counters kept in the same table (cg_get_option reads them,
// cg_set_option resets them): the launches of wino_dgrad_fused_kernel (winograd.hip) and of wino3_fused_k (wino3.hip), so that a test can
// tell that the fused path ran and not its fallback.  CG_SAMPLER_ATOMIC_LAUNCHES counts the other way round: the launches of
// bilinear_bwd_k (sampler.hip), the float-atomic fallback of the sampler's deterministic gather backward.
// CG_PACK_WIDE: 1 = the weight re-packing after every parameter update runs in its wide launches (pack_weight_ups2_wide_kernel and
// pack_weight_batch_wide_kernel in pack.hip, the both-operand Winograd filter transforms in winograd.hip), 0 = the kernels they replace.
// The bytes written are the same.
void opt_count(Opt o);

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Per-stream scratch of the deterministic column reductions (batch-norm statistics / backward sums, bias gradients): every
// workgroup writes its per-channel partials here, the LAST one to arrive (a ticket counter, kept at the front of the block and
// left at zero again) adds them up in a fixed order - no floating-point atomics, so a batch-norm layer gives the same bits on
// every run (the property the reference protects by pinning stn's sampler to the CPU, models.lua:889-899).  One block per
// stream out of a pool of eight allocated on the FIRST use of any stream (that one must be outside a graph capture; a stream that
// first appears inside a capture takes a pooled block without allocating).
constexpr size_t kColScratchBytes = 8u << 20;
void* col_scratch(hipStream_t stream);   // nullptr + cg::fail() on error
// ---- hardware queues (round 5).  The HIP runtime serves ALL streams of a process from GPU_MAX_HW_QUEUES = 4 hardware queues,
// assigned in creation order; two streams of one queue run back to back whatever the dependency graph says, and WHICH streams share a
// queue decides how much of a plan's overlap exists (measured: +-10 % per step between creation orders; one extra stream created by
// the library once moved the host's side stream onto the main stream's queue, +2.7 %; more than 4 queues is far worse - 8: 7.4 ms,
// 5: 11 ms per step against 5.9, the queues then time-slice the chip).  So side streams are not created where they are needed: they
// come out of one pool whose streams are CLASSIFIED, once, by a timing probe against the caller's stream (two spinning kernels on a
// pair of streams: together they take one kernel's time on different queues, two on the same), and a plan asks for "the k-th stream of
// queue class c": class 0 = the caller's own queue, 1..3 = the other three, numbered in the order the probe meets them.
hipStream_t queue_stream(hipStream_t ref, int cls, int slot);   // nullptr + cg::fail() on error
int queue_class(hipStream_t ref, hipStream_t s);                // class of a pool stream (or of ref itself: 0); -1 unknown

// ---- what gemm.hip, wgrad_finish.hip and pack.hip share ----------------------------------------------------------------------------
constexpr int MAXG = 4;  // groups per launch: same geometry, separate tensors (D32_st3's identical branches)
constexpr int kMaxStridedGroups = 36;   // ... or up to 36 equally spaced ones (cg_conv2d_wgrad_strided: 16 planes of F(2x2,3x3), 4 x 9 of F(2x2,2x2))
template <typename T>
__device__ __forceinline__ T sel4(int i, T a, T b, T c, T d) { return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d)); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float f4c(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
// the four-pointer fields of the kernel arguments (x0 .. x3 and their like: scalars, no arrays - runtime indexing would go to scratch)
// from an array of n <= MAXG group pointers
template <typename T>
static inline void set4(T& p0, T& p1, T& p2, T& p3, const T* src, int n) {
    T* const dst[MAXG] = {&p0, &p1, &p2, &p3};
    for (int i = 0; i < MAXG; ++i) *dst[i] = (src && i < n) ? src[i] : nullptr;
}
// upsample(2) -> conv k x k as four phase convolutions on the low-res input: canonical tap d of a k-tap kernel (pad p) seen from output
// phase a -> index of the low-res tap it folds into; kp = low-res taps per dimension
__device__ __host__ __forceinline__ int phase_map(int a, int d, int pad) { return ((a + d - pad) >> 1) - ((a - pad) >> 1); }
static inline int phase_kp(int k, int pad) { return phase_map(0, k - 1, pad) + 1; }

// The finish of a weight gradient (csrc/wgrad_finish.hip): what a weight-gradient launch left in its workspace and where it goes.
struct WgradParts {
    const float* part;        // [S][ngroups][P][taps * Cin][Cout]: P = 4 phases of kp x kp taps behind an upsampling, else 1 of kH x kW
    const float* bias_part;   // [S][ngroups][P][Cout] column sums of dy, or null: no bias gradient
    float* const* gw;         // canonical [Cout][Cin][kH][kW] per group, accumulated into
    float* const* gb;         // [Cout] per group; null, or null entries, where there is none
    long gws;                 // != 0: equally spaced groups, group g accumulates into gw[0] + g * gws
    int ngroups, S, Cin, Cout, kH, kW, pad, ups;
    float scale;
};
// defer: a small finish is queued on the stream for cg_conv2d_wgrad_flush, which runs all queued ones in one launch
int wgrad_finish(hipStream_t st, const WgradParts& w, bool defer);
// Drop every weight-gradient reduction still queued by cg_conv2d_wgrad_*_deferred (any stream): a pass that failed half way must not
// leave partial sums behind for the next flush to add to a gradient.
void wgrad_discard_all();

// 3x3 convolutions with <= 3 output planes as a scatter-form GEMM on the MFMA, input read once (csrc/skinny.hip, round 6): widths that
// are a multiple of 32 up to 128, 64 or 128 input planes.  CG_SKINNY: 1 = these where they apply (else round 1's VALU kernels in the
// same file), 2 = the VALU kernels always, 0 = the generic implicit GEMM.  gemm.hip decides which family runs.
constexpr int kSkinnyWgradBlocks = 512;   // partial planes of a skinny weight gradient, at most
bool skinny_ok(int ngroups, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups);   // a skinny layer at all (either family)
size_t skinny_wgrad_ws_bytes(int Cin, int Cout);
void skinny_valu_forward(hipStream_t st, const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout);
void skinny_valu_wgrad(hipStream_t st, const float* x, const float* dy, float* part, float* bias_part, int N, int H, int W, int Cin, int Cout,
                       int blocks, long ppb);
bool skinny_mfma_ok(int Cin, int Cout, int H, int W);
int skinny_mfma_forward(hipStream_t st, const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout);
int skinny_mfma_wgrad(hipStream_t st, const float* x, const float* dy, float* part, float* bias_part, int N, int H, int W, int Cin, int Cout,
                      int max_blocks);   // returns the number of partial planes written, -1 on error

// Fused-transform Winograd F(2x2,3x3) for plain 64 -> 64 plane 3x3 convolutions (csrc/wino3.hip, round 6).  CG_WINO3: 1 = where the
// geometry fits and the launch has >= 2 workgroups per CU, 2 = wherever the geometry fits (tests), 0 = never (the direct implicit GEMM).
// headwg.hip: weight gradient of nn.View -> nn.Linear on an NHWC map (T = H*W taps of C planes) straight into the canonical gradWeight
bool head_wgrad_ok(int N, int T, int C, int Co);
int head_wgrad(hipStream_t st, const float* x, const float* dy, float* gw, float* gb, int N, int T, int C, int Co, float scale);
// The transformed filters U (kWino3UFloats floats) ride behind the packed taps of such a layer's operands, at wf / wb + kWino3UOffset:
// cg_pack_conv_weight_floats() counts them, wino3_note_pack (called by cg_pack_conv_weight / _batch) writes them, wino3_forward reads them.
constexpr int kWino3UOffset = 9 * 64 * 64, kWino3UFloats = 16 * 64 * 64;
static inline bool wino3_layer(int Cout, int Cin, int kH, int kW) { return Cout == 64 && Cin == 64 && kH == 3 && kW == 3; }
bool wino3_geom_ok(int ngroups, int N, int H, int W, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups);
int wino3_note_pack(hipStream_t st, int n, const float* const* w, float* const* wf, float* const* wb, const int* Cout, const int* Cin,
                    const int* kH, const int* kW, const int* wb_map);
int wino3_forward(hipStream_t st, int ngroups, const float* const* x, const float* const* wpk, const float* const* bias, float* const* y,
                  int N, int H, int W);   // 1 launched, 0 not this path, -1 error

// grid for memory-bound grid-stride kernels: enough blocks to fill 256 CUs x 8
static inline int ew_grid(long n, int per_block = 256) {
    long b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    // kEwWgsPerCU = 4 (8 until round 4): beside a GEMM from another queue a memory-bound kernel waits for a slot per workgroup,
    // so fewer, longer-lived workgroups get through sooner - same-box step 6.36 -> 6.27 ms, alone no difference (profiles/r04_sweeps.txt)
    const long cap = (long)kNumCU * kEwWgsPerCU;
    if (b > cap) b = cap;
    return (int)b;
}

// The float4 form of a memory-bound kernel runs when the count it walks divides by 4 and every tensor consulted sits on a 16-byte
// boundary (a null pointer counts as aligned).  Which count and which tensors is each entry point's own business.
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <class... P>
static inline bool vec_ok(long n, const P*... p) { return n % 4 == 0 && (al16(p) && ...); }
// a grid-stride kernel over n lanes on the entry point's `stream`; nothing to launch for n <= 0
#define CG_EW_LAUNCH(kern, n, ...)                                                                    \
    do {                                                                                              \
        if ((n) > 0) {                                                                                \
            hipLaunchKernelGGL(kern, dim3(cg::ew_grid(n)), dim3(256), 0, cg::S(stream), __VA_ARGS__); \
            CG_LAUNCH_CHECK();                                                                        \
        }                                                                                             \
    } while (0)
// The float4-or-scalar twins of one kernel template over n floats: where `vec`, V = 4 and n / 4 lanes, else V = 1 and n lanes.  The
// kernel and its arguments are written once, with V wherever the width enters: as the template argument, and under every length or
// channel count that the kernel takes in lanes (none where the kernel itself walks the n % 4 floats behind its float4 body)
#define CG_EW_LAUNCH_V(vec, kern, n, ...)                                                                                   \
    do {                                                                                                                    \
        if ((n) > 0) {                                                                                                      \
            if (vec) { constexpr int V = 4; hipLaunchKernelGGL(kern, dim3(cg::ew_grid((n) / V)), dim3(256), 0, cg::S(stream), __VA_ARGS__); } \
            else { constexpr int V = 1; hipLaunchKernelGGL(kern, dim3(cg::ew_grid((n) / V)), dim3(256), 0, cg::S(stream), __VA_ARGS__); }    \
            CG_LAUNCH_CHECK();                                                                                              \
        }                                                                                                                   \
    } while (0)

// ---- device-side helpers -------------------------------------------------
// The fused-transform Winograd kernels (wino3.hip, wino_dgrad_fused_kernel in winograd.hip) read their A operand from an LDS patch with
// ds_read_b128, which the LDS serves in 16-lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (+32).  Row i of an MFMA tile (= lane & 31
// of the A operand) -> output tile (ty, tx) of a 4 x 8 block, ty = result >> 3, tx = result & 7: the first group takes tile rows 0, 1, the
// second 2, 3, so that a group covers two whole tile rows.
constexpr int tile_of_row_c(int l) {
    return ((l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? 0 : 16) +
           ((l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? (l < 4 ? l : (l < 16 ? l - 8 : l - 12)) : (l < 12 ? l - 4 : (l < 20 ? l - 8 : l - 16)));
}
__device__ __forceinline__ int tile_of_row(int l) {
    const bool ga = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
    const int rank = ga ? (l < 4 ? l : (l < 16 ? l - 8 : l - 12)) : (l < 12 ? l - 4 : (l < 20 ? l - 8 : l - 16));
    return (ga ? 0 : 16) + rank;
}
// Transformed filters of the fused Winograd 3x3 kernel (wino3.hip) for filter pair idx = co * 64 + ci of a 64 -> 64 plane layer:
// U[pos][ci / 4][co][4] = (G g G^T)[xi][nu], pos = xi * 4 + nu; uf: the forward's g = w[co][ci][:][:], ub: the data gradient's (planes
// swapped, taps flipped) g[a][b] = w[ci][co][2 - a][2 - b].  One body for wino3_pack_k and for the batch pack's own workgroups
// (pack_weight_batch_wide_kernel, pack.hip), so that both write the same bits.
__device__ __forceinline__ void wino3_pack_item(const float* __restrict__ w, float* uf, float* ub, int idx) {
    constexpr int C = 64;
    const int co = idx / C, ci = idx % C;
    const float G[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
    for (int flip = 0; flip < 2; ++flip) {
        float* U = flip ? ub : uf;
        if (!U) continue;
        float g[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) g[a][b] = flip ? w[((long)ci * C + co) * 9 + (2 - a) * 3 + (2 - b)] : w[((long)co * C + ci) * 9 + a * 3 + b];
        float t[4][3];
        for (int i = 0; i < 4; ++i)
            for (int b = 0; b < 3; ++b) t[i][b] = G[i][0] * g[0][b] + G[i][1] * g[1][b] + G[i][2] * g[2][b];
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k)
                U[(((long)(i * 4 + k) * (C / 4) + ci / 4) * C + co) * 4 + (ci & 3)] = t[i][0] * G[k][0] + t[i][1] * G[k][1] + t[i][2] * G[k][2];
    }
}
// the engine's counter-based generator: splitmix64 of (seed, counter), 24-bit mantissa uniform in [0,1)
// (host twin tensor.SplitMix, oracle twin orc_rng_u01)
__device__ __forceinline__ float u01(uint64_t seed, uint64_t ctr) {
    uint64_t z = seed + (ctr + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Cross-workgroup hand-over of the partial sums.  The eight XCDs have private L2s, so an agent-scope fence costs a write-back
// walk plus an invalidate of the XCD's whole L2; issued by every wave of every workgroup (__threadfence in all threads) that is
// 128 walks per XCD, serialised: +30 us on an 18 us reduction (measured).  CG_COL_HANDOVER picks the protocol:
//   0  __threadfence() in every thread on both sides (the textbook form)
//   3  one release fence per WORKGROUP (thread 0, after the barrier that orders the other waves' stores before it - fences are
//      cumulative), one acquire fence per wave of the finishing workgroups only
//   4  no fences: partials are published and read with returning agent-scope atomics (swap / or-with-zero), which execute at the
//      device's coherence point like the double atomicAdds this replaces
// Same box, ms per step: 0 = 7.23, 3 = 7.13 - 7.16, 4 = 7.12 - 7.15 (profiles/r03_colreduce_handover.txt).  A fence-free form with
// write-through (sc1) stores / sc1 loads and only s_waitcnt in front of the ticket measured 7.10 - 7.13 but is NOT covered by the
// documented memory model (is a store's vmcnt acknowledgement its visibility to the other XCDs?) and failed parity runs that a
// later-found host-side race (the scratch's memset against non-blocking streams, see col_scratch) may or may not explain: not shipped.
#ifndef CG_COL_HANDOVER
#define CG_COL_HANDOVER 3
#endif
__device__ __forceinline__ void st_agent(double* p, double v) {
#if CG_COL_HANDOVER == 4
    const unsigned long long old = __hip_atomic_exchange((unsigned long long*)p, (unsigned long long)__double_as_longlong(v),
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"v"(old));   // keep the returning form: its s_waitcnt means the swap has been performed
#else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ double ld_agent(const double* p) {
#if CG_COL_HANDOVER == 4
    unsigned long long zero = 0ull;
    asm volatile("" : "+v"(zero));   // opaque, or the compiler turns the idempotent read-modify-write into a plain load
    return __longlong_as_double((long long)__hip_atomic_fetch_or((unsigned long long*)const_cast<double*>(p), zero, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT));
#else
    return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// true in exactly one workgroup of the grid: the last one to arrive at this point.  What the others published with st_agent before
// their arrival is visible to its ld_agent loads.  counter must be zero before the launch; the last workgroup leaves it at zero again.
__device__ __forceinline__ bool last_block_arrives(unsigned* counter, unsigned total) {
    __shared__ int last_flag;
#if CG_COL_HANDOVER == 0
    __threadfence();
#else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
    if (threadIdx.x == 0) {
#if CG_COL_HANDOVER == 3
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = (t == total - 1) ? 1 : 0;
        if (last_flag) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
#if CG_COL_HANDOVER == 0
    if (last_flag) __threadfence();
#elif CG_COL_HANDOVER == 3
    if (last_flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
    return last_flag != 0;
}

// ---- second stage of the deterministic column reductions ------------------------------------------------------------
// A launch of `chunks` row chunks leaves chunks x nk fp64 partials.  Adding them in ONE workgroup costs chunks dependent-latency
// loads per column (measured: 256 chunks = 90 us on the tail of an 18 us kernel), so the sum is a fixed two-level tree: chunks are
// grouped G at a time, the last workgroup to arrive of a GROUP adds its G rows (16 loads in flight per column) into the group's row,
// the last group to finish adds the group rows.  Which workgroup does a sum depends on timing, the ORDER of every addition does not.
struct ColTree {
    int G, ngroups;
    unsigned* counters;   // [0] groups finished, [1 + g] arrivals of group g; all zero between launches
    double* part;         // [chunks][nk]
    double* grp;          // [ngroups][nk]
    double* extra;        // caller-defined tail (e.g. the PReLU slope partials)
};
constexpr int kColTreeMaxGroups = 32;
static inline bool col_tree_layout(char* scr, long chunks, size_t nk, size_t nextra, ColTree& t) {
    t.G = (int)std::max<long>(16, (chunks + kColTreeMaxGroups - 1) / kColTreeMaxGroups);
    t.ngroups = (int)((chunks + t.G - 1) / t.G);
    t.counters = (unsigned*)scr;
    t.part = (double*)(scr + 256);
    t.grp = t.part + (size_t)chunks * nk;
    t.extra = t.grp + (size_t)t.ngroups * nk;
    return 256 + sizeof(double) * ((size_t)chunks * nk + (size_t)t.ngroups * nk + nextra) <= kColScratchBytes;
}

// out[k] = rows[0][k] + rows[1][k] + ... in row order, loads 16 rows ahead of the additions (rows published with st_agent)
__device__ __forceinline__ void col_sum_rows(const double* rows, int nrows, int nk, double* out) {
    for (int k = threadIdx.x; k < nk; k += blockDim.x) {
        double t = 0.0;
        int y = 0;
        for (; y + 16 <= nrows; y += 16) {
            double v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = ld_agent(&rows[(size_t)(y + j) * nk + k]);
#pragma unroll
            for (int j = 0; j < 16; ++j) t += v[j];
        }
        for (; y < nrows; ++y) t += ld_agent(&rows[(size_t)y * nk + k]);
        st_agent(&out[k], t);
    }
}

// called by every workgroup after it stored its partial row (chunk = its row chunk, blocks_per_chunk = workgroups sharing a chunk);
// true in the one workgroup that wrote the final sums
__device__ __forceinline__ bool col_tree_finish(const ColTree& t, int chunk, int chunks, unsigned blocks_per_chunk, int nk, double* sums) {
    const int g = chunk / t.G;
    const int in_group = min(t.G, chunks - g * t.G);
    if (!last_block_arrives(t.counters + 1 + g, (unsigned)in_group * blocks_per_chunk)) return false;
    col_sum_rows(t.part + (size_t)g * t.G * nk, in_group, nk, t.grp + (size_t)g * nk);
    if (!last_block_arrives(t.counters, (unsigned)t.ngroups)) return false;
    col_sum_rows(t.grp, t.ngroups, nk, sums);
    return true;
}

// block-wide sum for 256-thread blocks; result valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* sh /*[4]*/) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return r;
}

// ---- element arithmetic of the memory-bound kernels ------------------------------------------------------------------
// ops.hip, fused.hip, the GEMM epilogue (gemm.hip) and the localisation launch (locnet.hip) promise each other's bits: a fused kernel
// those of the kernels it replaces, a float4 kernel those of its scalar twin.  They hold because every expression below is written
// ONCE and every twin is one template over Vec<VW>.  The build contracts a * b + c into an fma where the product feeds the sum
// directly; an edit here moves all users together.
#define CG_GRID_STRIDE(i, n) \
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// VW floats of one lane: one 16-byte access at VW == 4 (the pointer must be 16-byte aligned), one dword at VW == 1.  T is the raw lane
// type with its operations as static functions: bilinear_bwd_det_k (sampler.hip) keeps its register arrays in T, and from arrays of a
// wrapping struct the compiler forms other code - and, where it fuses a product into a sum, other bits (found with the pins of
// tests/test_gpu_membound_bits.py).  The elementwise kernels hold one Vec and address its lanes with [].  dot() and fma() state their
// operation order; their arguments are taken by value for the same reason.
template <int VW> struct Vec;
template <> struct Vec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, T v) { *p = v; }
    static __device__ __forceinline__ float dot(T a, T b) { return a * b; }
    static __device__ __forceinline__ void fma(T& acc, float w, T g) { acc += w * g; }
    T v;
    __device__ __forceinline__ float& operator[](int) { return v; }
    __device__ __forceinline__ float operator[](int) const { return v; }
    // lane i of a tensor; per-channel parameter c
    static __device__ __forceinline__ Vec load(const float* p, long i) { return Vec{p[i]}; }
    __device__ __forceinline__ void store(float* p, long i) const { p[i] = v; }
    static __device__ __forceinline__ Vec ldc(const float* p, int c) { return Vec{p[c]}; }
};
template <> struct Vec<4> {
    typedef float4 T;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ void st(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
    static __device__ __forceinline__ float dot(T a, T b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
    static __device__ __forceinline__ void fma(T& acc, float w, T g) { acc.x += w * g.x; acc.y += w * g.y; acc.z += w * g.z; acc.w += w * g.w; }
    T v;
    __device__ __forceinline__ float& operator[](int k) { return (&v.x)[k]; }
    __device__ __forceinline__ float operator[](int k) const { return (&v.x)[k]; }
    // lane i of a tensor walked four floats at a time; per-channel parameters are views into the flat parameter vector (any 4-byte
    // alignment): four scalar loads of channels 4 c ..
    static __device__ __forceinline__ Vec load(const float* p, long i) { return Vec{ld(p + 4 * i)}; }
    __device__ __forceinline__ void store(float* p, long i) const { st(p + 4 * i, v); }
    static __device__ __forceinline__ Vec ldc(const float* p, int c) { return Vec{make_float4(p[4 * c], p[4 * c + 1], p[4 * c + 2], p[4 * c + 3])}; }
};

// act: 0 identity, 1 PReLU, 2 LeakyReLU.  The side of the kink is decided here and nowhere else: x itself passes through LeakyReLU
// unscaled (x >= 0) and takes PReLU's slope (x > 0 fails), for the value and for the derivative alike
__device__ __forceinline__ bool act_passes(int act, float x) { return act == 0 || (act == 1 ? x > 0.f : x >= 0.f); }
__device__ __forceinline__ float act(int act, float v, float a) { return act_passes(act, v) ? v : a * v; }
// d(act)/dx at x applied to an incoming gradient d
__device__ __forceinline__ float dact(int act, float x, float d, float a) { return act_passes(act, x) ? d : a * d; }
// PReLU's slope gradient: s += sum over the lanes of (x <= 0 ? x d : 0).  Each width keeps its own sequence of roundings, which the
// pins of tests/test_gpu_membound_bits.py hold: one lane fuses its product into the running sum and adds nothing for x > 0; four lanes
// round their products, add them left to right (zeros for x > 0) and add that to the running sum.
__device__ __forceinline__ float slope_term(float x, float d) { return x <= 0.f ? x * d : 0.f; }
template <int VW>
__device__ __forceinline__ void slope_acc(float& s, const Vec<VW>& x, const Vec<VW>& d) {
    if constexpr (VW == 1) {
        if (x[0] <= 0.f) s = fmaf(x[0], d[0], s);
    } else {
        float t = slope_term(x[0], d[0]);
#pragma unroll
        for (int k = 1; k < VW; ++k) t += slope_term(x[k], d[k]);
        s += t;
    }
}
// PReLU backward of one workgroup's lanes of a grid-stride walk over n lanes of VW floats: dx = x > 0 ? dy : a dy, and, where
// `partial` is given, the workgroup's slope-gradient sum into it (cg_prelu_backward: x, dy, dx whole; cg_prelu_backward_grouped: at
// the group's base with the group's slope)
template <int VW>
__device__ __forceinline__ void prelu_bwd_walk(const float* x, const float* dy, float a, float* dx, long n, double* partial) {
    __shared__ double sh[4];
    float s = 0.f;
    CG_GRID_STRIDE(i, n) {
        const Vec<VW> v = Vec<VW>::load(x, i), g = Vec<VW>::load(dy, i);
        Vec<VW> o;
#pragma unroll
        for (int k = 0; k < VW; ++k) o[k] = dact(1, v[k], g[k], a);
        o.store(dx, i);
        slope_acc(s, v, g);
    }
    if (!partial) return;
    const double t = block_sum_256((double)s, sh);
    if (threadIdx.x == 0) *partial = t;
}
// the sum of such partials by one workgroup of 256 in a fixed order; valid in thread 0
__device__ __forceinline__ double partials_sum_256(const double* part, int nparts) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    return block_sum_256(s, sh);
}
// batch norm: xhat, y = xhat gamma + beta, dx = gamma invstd (dy - mean(dy) - xhat mean(dy xhat))
__device__ __forceinline__ float bn_xhat(float x, float m, float s) { return (x - m) * s; }
__device__ __forceinline__ float bn_norm(float x, float m, float s, float g, float b) { return bn_xhat(x, m, s) * g + b; }
__device__ __forceinline__ float bn_dx(float x, float dy, float g, float m, float s, float m1, float m2) {
    return g * s * (dy - m1 - bn_xhat(x, m, s) * m2);
}
// the augmentation's noise value of one source sample (images.hip's on-the-fly kernels, faces.hip's offline variants): Irwin-Hall sum
// of the twelve 16-bit fields of three splitmix64 outputs (exact in fp32)
__device__ __forceinline__ float augment_noise(uint64_t seed, uint64_t ctr) {
    unsigned S = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint64_t z = seed + (ctr + k + 1) * 0x9E3779B97F4A7C15ull;   // common.h u01's generator, all 64 bits of it
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        S += (unsigned)(z & 0xFFFF) + (unsigned)((z >> 16) & 0xFFFF) + (unsigned)((z >> 32) & 0xFFFF) + (unsigned)(z >> 48);
    }
    return (float)((int)S - 393210) * (1.0f / 65536.0f);   // |S - 393210| < 2^24 and a power of two: both steps exact
}
// tf.warp(order 1, mode="nearest") as the augmentation kernels (images.hip) and the face extraction (faces.hip) restate it in fp32:
// one axis of the warp's source position: clamped to [0, L-1] (NaN -> 0), split into the two taps and the fraction
__device__ __forceinline__ void warp_taps(float s, int L, int* i0, int* i1, float* f) {
#pragma clang fp contract(off)
    const float hi = (float)(L - 1);
    s = !(s >= 0.f) ? 0.f : (s > hi ? hi : s);
    *i0 = (int)s;
    *f = s - (float)*i0;
    *i1 = min(*i0 + 1, L - 1);
}
// ---- the spatial transformer's affine arithmetic: sampler.hip's cg_affine_* kernels and the fused launches of locnet.hip ----------
// Each expression stands once, with the parenthesisation and operand order the pins of tests/test_gpu_membound_bits.py recorded.
// coordinate of index i of n in [-1, 1]
__device__ __forceinline__ float grid_coord(int i, int n) { return n > 1 ? -1.f + 2.f * (float)i / (float)(n - 1) : -1.f; }
// The transform's parameters as the generator stores them - [theta][scale][tx, ty], each part present by its flag - unpacked, and
// T = R(theta) * S(s) * Tr(tx,ty); rows: [c*s, -sn*s, c*s*tx - sn*s*ty], [sn*s, c*s, sn*s*tx + c*s*ty].  cs, where given, receives
// (cos, sin, scale, tx, ty) for affine_param_grad.  Unpacking and T are ONE function on purpose: a caller that wants only cs leaves T
// unused, and with a separate unpacking the compiler contracts affine_param_grad's sums otherwise (profiles/locnet_stages_resources.txt)
__device__ __forceinline__ void affine_T(const float* prm, int ur, int us, int ut, float* T, float* cs = nullptr) {
    int k = 0;
    float th = 0.f, sc = 1.f, tx = 0.f, ty = 0.f;
    if (ur) th = prm[k++];
    if (us) sc = prm[k++];
    if (ut) { tx = prm[k]; ty = prm[k + 1]; }
    const float c = cosf(th), s = sinf(th);
    T[0] = c * sc; T[1] = -s * sc; T[2] = c * sc * tx - s * sc * ty;
    T[3] = s * sc; T[4] = c * sc;  T[5] = s * sc * tx + c * sc * ty;
    if (cs) { cs[0] = c; cs[1] = s; cs[2] = sc; cs[3] = tx; cs[4] = ty; }
}
// gparams from g = dL/dT
__device__ __forceinline__ void affine_param_grad(float c, float s, float sc, float tx, float ty, const float* g, int ur, int us, int ut, float* gp) {
    int k = 0;
    if (ur) {
        // d/dtheta: c -> -s, s -> c
        const float d0 = -s * sc, d1 = -c * sc, d2 = -s * sc * tx - c * sc * ty;
        const float d3 = c * sc, d4 = -s * sc, d5 = c * sc * tx - s * sc * ty;
        gp[k++] = g[0] * d0 + g[1] * d1 + g[2] * d2 + g[3] * d3 + g[4] * d4 + g[5] * d5;
    }
    if (us) gp[k++] = g[0] * c + g[1] * (-s) + g[2] * (c * tx - s * ty) + g[3] * s + g[4] * c + g[5] * (s * tx + c * ty);
    if (ut) {
        gp[k] = g[2] * (c * sc) + g[5] * (s * sc);
        gp[k + 1] = g[2] * (-s * sc) + g[5] * (c * sc);
    }
}
// one grid point's terms of gT[r][:] = sum_{i,j} ggrid[i,j,r] * (y_i, x_j, 1): fp32 products into fp64 sums
__device__ __forceinline__ void affine_grid_acc(double (&acc)[6], float g0, float g1, float y, float x) {
    acc[0] += g0 * y; acc[1] += g0 * x; acc[2] += g0;
    acc[3] += g1 * y; acc[4] += g1 * x; acc[5] += g1;
}

}  // namespace cg
