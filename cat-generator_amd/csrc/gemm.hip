// Implicit-GEMM convolution / linear kernels on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces the THNN/THCUNN/cudnn kernels the reference reaches through
// cudnn.SpatialConvolution (models.lua:206,212,218,222), nn.SpatialConvolution
// (models.lua:646-685,844-846) and nn.Linear (models.lua:199,697,700,850,853):
//   igemm_nn : updateOutput and updateGradInput  (Y[m][n] = sum_k A(m,k) W[k][n])
//   igemm_tn : accGradParameters                 (dW[k][n] = sum_m A(m,k) dY[m][n], as split partial sums: wgrad_finish.hip reduces them)
// A(m,k) is never materialised: m -> grid pixel (n,oy,ox), k -> (tap,ci), gathered from the NHWC tensor.
//
// nn.SpatialUpSamplingNearest(2) -> conv (models.lua:205-206,211-212,217-218) is executed as FOUR PHASE
// CONVOLUTIONS on the low-resolution input: output pixel (2i+a, 2j+b) only ever sees ceil((k+1)/2)^2 distinct
// low-res taps, so the k x k weights are pre-summed per phase (a,b) into k' x k' kernels (k'=2 for k=3, 3 for
// k=5): 2.25x / 2.78x fewer MACs than convolving the materialised upsampled map, identical up to fp32
// re-association of the weight sums (the packs: pack.hip).  The data gradient w.r.t. the low-res input (upsampling's 2x2 block sum
// folded in) is ONE GEMM over the 4 phases' taps; the weight gradient is taken per phase and mapped back onto
// the canonical taps by the finish (wgrad_finish.hip).
//
// fp32 MFMA issues at exactly the fp32 VALU rate, so every VALU instruction in the main loop costs MFMA
// throughput (measured: 4.9 VALU per MFMA = 73 % pipe utilisation).  The FAST path therefore keeps the gather
// lean: tap bookkeeping lives in SGPRs, per-row validity is a precomputed 64-bit tap mask, and loads are
// buffer_load_dwordx4 whose out-of-range offset returns 0 (no branches, no zero-fills).
//
// Tiling (wave64, 4 waves / workgroup): block tile BM x BN, K step 16 or 32, each wave owns MI x NI MFMA 32x32
// accumulators; LDS tiles are double buffered, one barrier per K tile.  How a K tile gets into LDS:
//   * igemm_nn_kernel / igemm_tn_kernel (register staging): both operands K-major in LDS ([k][m] XOR-swizzled, [k][n]),
//     a fragment read is one conflict-free ds_read_b32 per operand per MFMA; the next tile's global loads are issued
//     before the current tile's MFMAs and stored to LDS behind them.  (The k-quad LDS layouts, the loads two tiles ahead and the
//     quad weight-gradient kernel of rounds 2-4 lost every A/B they were in and were removed in round 5: profiles/NOTES_r01_r02.md.)
//   * igemm_nng_kernel / igemm_tng_kernel (LDS-direct loads, buffer_load_dwordx4 ... lds): the default where the
//     geometry allows (round 2: the ablation builds below located the loop's loss in the register -> LDS staging).
// What the two staging families of a GEMM have in common is written once: the blockIdx.z decode and operand selection (nn_tile / tn_tile),
// the NN epilogue (nn_epilogue: bias, activation, statistics, the lean and the generic stores), the TN partial store (tn_store_partials) and
// the host's packing of the four-pointer argument fields (set4) here; in gemm_tile.h everything in front of and inside the K loop - the
// XCD tile orders (nn_tile_order / tn_tile_order), the FAST gather state of the NN pair (NNGather: row decode, tap masks, the tap walk
// with its position-major variant, weight offsets, descriptors), the lean addressing of the TN pair (tn_col_decode, tn_lean_geom - the
// rule the host's tng_ok states too -, tn_lean_a / tn_lean_b, tn_tile_bases), the two-buffer loop driver (k_loop2) and the K-major
// fragment loop (mfma_k_major; igemm_nng_kernel's quad fragments are its own).  The host picks the compiled block tile in one place
// (with_block_tile).  The skinny 3x3 layers (<= 3 output planes) have their kernels, MFMA and
// VALU, in skinny.hip; this file only decides which of them runs (cg::skinny_ok, CG_SKINNY).  What follows a weight-gradient launch - the
// reduction of its partials into the canonical gradients, now or deferred - is cg::wgrad_finish (wgrad_finish.hip); the re-packing of the
// canonical weights into this file's operands is pack.hip.
#include "common.h"
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

using cg::f4c;
using cg::kMaxStridedGroups;
using cg::ld4;
using cg::MAXG;
using cg::phase_kp;
using cg::sel4;
using cg::set4;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 16;
constexpr unsigned OOB = 0x80000000u;
// -DCG_TRACE (CG_BUILD_DEFINES=-DCG_TRACE, build.py): every igemm_nn_kernel workgroup records 100 MHz timestamps at its start, behind
// the prologue (first tile in LDS), behind the K loop and at its end, plus the hardware id of the CU it ran on, into the
// buffer handed to cg_debug_set_trace - scripts/wg_trace.py turns that into the dispatch balance and the phase times.
#ifdef CG_TRACE
__device__ unsigned long long* g_trace;
#define CG_STAMP(slot)                                                                                                  \
    do {                                                                                                                \
        if (threadIdx.x == 0 && g_trace) {                                                                              \
            const long wg = blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z);                  \
            g_trace[wg * 8 + (slot)] = wall_clock64();                                                                  \
            if ((slot) == 0) {                                                                                          \
                g_trace[wg * 8 + 4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  /* HW_REG_HW_ID */                     \
                g_trace[wg * 8 + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 20); /* HW_REG_XCC_ID */                    \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
#else
#define CG_STAMP(slot) do { } while (0)
#endif  // >= num_records of every descriptor below: the load returns 0

// tap t of a launch -> (ty, tx, element offset):  group = t / kk, (ry,rx) = (t % kk) / kw, % kw
//   phase bits (a,b) = launch phase (nphase == 4)  or  group bits (ngroups == 4)  or  0
//   ty = sgn*(r0y(a)+ry), tx = sgn*(r0x(b)+rx);  source pixel = ((oy+ty)*ss + a*(ss==2), (ox+tx)*ss + b*(ss==2))
struct TapDesc {
    int kw, kk, ngroups, sgn, ss;
    int r0y0, r0y1, r0x0, r0x1;   // tap origin per phase bit (no arrays: runtime indexing would go to scratch)
};

struct Geom {
    int M;                 // grid pixels per phase: N*Hg*Wg
    int Hg, Wg;            // grid per image
    int lgW, lgHW;         // log2(Wg), log2(Hg*Wg) when both are powers of two, else -1
    int Hv, Wv;            // (oy+ty, ox+tx) must lie in [0,Hv) x [0,Wv)
    int Hs, Ws;            // source tensor spatial dims
    int Cin, Cout;         // GEMM K-channels / N
    int so, Hout, Wout;    // grid pixel -> (n, oy*so+a, ox*so+b) of an [N,Hout,Wout] tensor (NN: y; TN: dy)
    int nphase;            // 1 or 4 (blockIdx.z)
    int ntaps, Ktot;       // per phase; Ktot = ntaps*Cin
    TapDesc td;
    int minoff0, minoff1, minoff2, minoff3;   // per phase: min(0, smallest tap element offset) - host-computed (finish_geom), the kernels' descriptor base
    // POSITION-MAJOR rows (round 5; igemm_nng_kernel<..., PM>): pmn = N (a power of two, a multiple of the row tile) puts grid pixel
    // (n, oy, ox) at row m = (oy * Wg + ox) * N + n, so that a row tile holds ONE pixel position of 64 images and all its rows share
    // their zero-padding taps, which the K loop then skips (D32_st3's 7x7 layer at 8x8: 38 % of the MACs multiply padding).  0 = the
    // image-major order everywhere else.  Split partials are in row order either way; out_row() maps a row to its output pixel.
    int pmn, pm_lg;
};

struct NNArgs {
    const float* x0; const float* x1; const float* x2; const float* x3;   // per group (no arrays: see TapDesc)
    const float* w0; const float* w1; const float* w2; const float* w3;   // [nphase][Ktot][Cout]
    const float* b0; const float* b1; const float* b2; const float* b3;   // [Cout] or null
    float* y0; float* y1; float* y2; float* y3;                           // output tensors
    float* part;        // split partials [S][ngroups*nphase][M][Cout] (nsplit > 1)
    int ngroups;
    Geom g;
    int kchunk;         // K range per split (multiple of BK)
    int nsplit;
    // fused epilogue (cg_conv2d_forward_ex): act 0 none, 1 PReLU (slope read from al<group>), 2 LeakyReLU (slope);
    // z<group> receives act(y) while y keeps the pre-activation (what the activation's backward needs).
    int act;
    float slope;
    const float* al0; const float* al1; const float* al2; const float* al3;
    float* z0; float* z1; float* z2; float* z3;
    // stats != null: per (phase, row tile, wave row) column sums of y and y^2 -> stats[row][2][Cout] (batch-norm statistics
    // of the layer behind this convolution, models.lua:206-207; single group, unsplit launches only)
    float* stats;
    int xcd_swizzle;
};

struct TNArgs {
    const float* x0; const float* x1; const float* x2; const float* x3;
    const float* d0; const float* d1; const float* d2; const float* d3;   // dy per group
    int ngroups;
    float* part;        // [S][ngroups*nphase][Ktot][Cout]
    float* bias_part;   // [S][ngroups*nphase][Cout] column sums of dy (gradBias partials) or null
    Geom g;
    int pchunk;         // pixels per split (multiple of BK)
    int xcd_swizzle;
    int pm_n;           // igemm_tng_kernel mode 2 (position-major K tiles): images per launch, a multiple of BK
    long xgs, dgs;      // != 0: group g reads x0 + g * xgs / d0 + g * dgs (up to kMaxStridedGroups equally spaced groups: the
                        // Winograd-domain weight-gradient GEMMs of winograd.hip in one launch), x1.. / d1.. unused
};


// blockIdx.z = group * nphase + phase of every GEMM launch, phase bits (pa, pb); with the operands of that group (w: this phase's kernel)
struct ZTile { int group, phase, pa, pb; };
struct NNTile : ZTile { const float* x; const float* bias; float* y; const float* w; };
struct TNTile : ZTile { const float* x; const float* dy; };
__device__ __forceinline__ ZTile z_decode(const Geom& g, int zz) {
    const int group = g.nphase == 1 ? zz : (g.nphase == 4 ? zz >> 2 : zz / g.nphase);
    const int phase = zz - group * g.nphase;
    return {group, phase, phase >> 1, phase & 1};
}
__device__ __forceinline__ NNTile nn_tile(const NNArgs& a, int zz) {
    const ZTile z = z_decode(a.g, zz);
    return {z, sel4(z.group, a.x0, a.x1, a.x2, a.x3), sel4(z.group, a.b0, a.b1, a.b2, a.b3), sel4(z.group, a.y0, a.y1, a.y2, a.y3),
            sel4(z.group, a.w0, a.w1, a.w2, a.w3) + (long)z.phase * a.g.Ktot * a.g.Cout};
}
__device__ __forceinline__ TNTile tn_tile(const TNArgs& a, int zz) {
    const ZTile z = z_decode(a.g, zz);
    return {z, a.xgs ? a.x0 + (long)z.group * a.xgs : sel4(z.group, a.x0, a.x1, a.x2, a.x3),
            a.dgs ? a.d0 + (long)z.group * a.dgs : sel4(z.group, a.d0, a.d1, a.d2, a.d3)};
}


typedef float f32x4 __attribute__((ext_vector_type(4)));
// NOTE: cast the WHOLE vector.  Extracting the four dwords one by one (bit_cast(float, v.x) ...) makes LLVM's
// InstCombine (ROCm 7.2, -O3) narrow the v4i32 buffer load to a single i32 and splat it - a silent miscompile.
__device__ __forceinline__ float4 bufld4(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    const f32x4 f = __builtin_bit_cast(f32x4, v);
    return make_float4(f.x, f.y, f.z, f.w);
}

// buffer_load_dwordx4 ... lds: lane l's 16 bytes go to lds + 16 l (lds wave-uniform), zeros for an out-of-range voff.
// The builtin exists in the device pass only (the host pass would silently drop the kernel's launch stub).
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t r, float* lds, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
#endif
}

__host__ __device__ __forceinline__ void tap_decode(const Geom& g, int t, int pa, int pb, int& ty, int& tx, int& off) {
    const TapDesc& d = g.td;
    const int grp = d.ngroups > 1 ? t / d.kk : 0;
    const int tt = t - grp * d.kk;
    const int ry = tt / d.kw, rx = tt - (tt / d.kw) * d.kw;
    int a = pa, b = pb;
    if (d.ngroups > 1) { a = grp >> 1; b = grp & 1; }
    ty = d.sgn * ((a ? d.r0y1 : d.r0y0) + ry);
    tx = d.sgn * ((b ? d.r0x1 : d.r0x0) + rx);
    const int ay = d.ss == 2 ? a : 0, ax = d.ss == 2 ? b : 0;
    off = ((ty * d.ss + ay) * g.Ws + (tx * d.ss + ax)) * g.Cin;
}

__device__ __forceinline__ void pix_decode(const Geom& g, int m, int& n, int& oy, int& ox) {
    if (g.lgW >= 0) {
        n = m >> g.lgHW;
        oy = (m >> g.lgW) & (g.Hg - 1);
        ox = m & (g.Wg - 1);
    } else {
        const int hw = g.Hg * g.Wg;
        n = m / hw;
        const int r = m - n * hw;
        oy = r / g.Wg;
        ox = r - oy * g.Wg;
    }
}

// element offset of grid pixel m (phase bits pa,pb) in the [N,Hout,Wout,Cout] tensor
__device__ __forceinline__ long out_row(const Geom& g, int m, int pa, int pb) {
    if (g.pmn) return ((long)(m & (g.pmn - 1)) * (g.Hg * g.Wg) + (m >> g.pm_lg)) * g.Cout;   // so == 1, nphase == 1 (host)
    if (g.so == 1 && g.nphase == 1) return (long)m * g.Cout;
    int n, oy, ox;
    pix_decode(g, m, n, oy, ox);
    return ((long)(n * g.Hout + oy * g.so + pa) * g.Wout + ox * g.so + pb) * g.Cout;
}

// position-major launches (Geom::pmn): the number of taps of a plain convolution that fall inside the image at pixel position pos.
// A tile at that position walks them in cdiv(taps * Cin, kchunk) equal K units (igemm_nng_kernel<..., PM>); the reduce adds as many.
__device__ __forceinline__ int pm_valid_taps(const Geom& g, int pos) {
    const TapDesc& d = g.td;
    const int kh = d.kk / d.kw;
    const int oy = g.lgW >= 0 ? pos >> g.lgW : pos / g.Wg, ox = pos - oy * g.Wg;
    const int ylo = d.sgn > 0 ? d.r0y0 : -(d.r0y0 + kh - 1), xlo = d.sgn > 0 ? d.r0x0 : -(d.r0x0 + d.kw - 1);
    const int vy = min(g.Hv - 1 - oy, ylo + kh - 1) - max(-oy, ylo) + 1;
    const int vx = min(g.Wv - 1 - ox, xlo + d.kw - 1) - max(-ox, xlo) + 1;
    return max(vy, 0) * max(vx, 0);
}

// Column XOR of the K-major A tile, as a function of the k quad kv = k / 4: a half-wave of the transposed store holds
// (K step / 4) quads x (128 / K step) consecutive rows and must land in 32 distinct banks; a fragment read (32 consecutive
// rows at fixed k) must stay a permutation of them.  K step 16: 4 quads x 8 rows -> flip row bits 3,4; K step 32: 8 quads x 4
// rows -> flip row bits 2,3,4 (PMC: the bits-3,4 form gave the K-step-32 kernel 10 % LDS bank-conflict cycles).
template <int BKT>
__device__ __forceinline__ int a_swizzle(int kv) { return BKT == 32 ? ((kv & 7) << 2) : ((kv & 3) << 3); }

#include "gemm_tile.h"   // tile order, NN gather state, TN addressing, the K loop: shared by the staging families below

// Lean epilogue of the NN kernels for a FULL tile whose output rows are consecutive ([row][Cout], i.e. stride-1 layers and split
// partials): one buffer store per value at (per-lane byte offset) + (row offset in an SGPR).  The generic loop below it - bounds checks,
// 64-bit addresses and an output-row decode per row - is ~2000 instructions per wave; with all workgroups of a launch reaching their
// epilogue together that was 10 us in which no MFMA ran (profiles/r03_wg_timeline_nn_kernels.txt).
template <int MI, int NI, bool ACT>
__device__ __forceinline__ void nn_store_lean(const f32x16 (&acc)[MI][NI], const float (&bj)[NI], float* ybase, float* zbase, unsigned vo,
                                              int c4, int act, float aslope) {
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)ybase, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)(ACT ? zbase : ybase), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (i * 32 + (r & 3) + 8 * (r >> 2)) * c4;   // wave-uniform
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const float v = acc[i][j][r] + bj[j];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ry, (int)(vo + j * 128), soff, 0);
                if (ACT) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(cg::act(act, v, aslope)), rz, (int)(vo + j * 128), soff, 0);
            }
        }
    }
}

// batch-norm statistics of a wave's columns -> a.stats[srow][2][Cout]; the two half-waves hold the two row halves of the same columns.
// GUARD: the tile may reach past Cout.
template <int BM, int WM, int WN, int NI, bool GUARD>
__device__ __forceinline__ void nn_store_stats(const NNArgs& a, const float (&s1)[NI], const float (&s2)[NI], int zz, int tm, int wave, int ncol, int h) {
    const Geom& g = a.g;
    const int srow = (zz * (int)((g.M + BM - 1) / BM) + tm) * WM + wave / WN;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const float t1 = s1[j] + __shfl_xor(s1[j], 32, 64), t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
        const int n = ncol + j * 32;
        if (h == 0 && (!GUARD || n < g.Cout)) {
            a.stats[((long)srow * 2 + 0) * g.Cout + n] = t1;
            a.stats[((long)srow * 2 + 1) * g.Cout + n] = t2;
        }
    }
}

// Epilogue of both NN kernels: D[i][j], i = (r&3) + 8*(r>>2) + 4*h (pixel), j = l31 (channel).  Bias, fused activation (second output),
// batch-norm statistics; split launches store their partials.  The stores, cheapest first: position-major lean (PM kernels only) ->
// consecutive lean -> strided lean (STRIDED: the LDS-direct kernel only) -> the generic bounds-checked loop.
// The arguments come BY VALUE, as the kernel holds them: through a reference the compiler merges the two loads of the slope into one load
// through a pointer that may point into the argument copy, and that copy then stays in scratch (8 bytes per lane in every NN kernel).
template <int BM, int BN, int WM, int WN, bool STRIDED, bool PM>
__device__ __forceinline__ void nn_epilogue(const f32x16 (&acc)[BM / WM / 32][BN / WN / 32], const NNArgs a, const NNTile z, int m0, int n0, int wm0,
                                            int wn0, int l31, int h, int wave, int tm, int zz, int split, int pos_u) {
    // Floating-point contraction is off in the epilogue, and the statistics' sum of squares states its own rounding: s2 = fma(v, v, s2) in
    // the strided loop and in the generic loop of the 32-column wave tiles (NI == 1), s2 + v * v (two roundings) in the generic loop of
    // the 64-column ones (NI == 2).  The bits of a batch-norm layer are part of what the parity tests pin (tests/test_gpu_gemm_bits.py).
#pragma clang fp contract(off)
    constexpr int MI = BM / WM / 32, NI = BN / WN / 32;
    const Geom& g = a.g;
    const int group = z.group, pa = z.pa, pb = z.pb;
    const float* gbias = z.bias;
    const bool partial = a.nsplit > 1;
    const bool add_bias = (gbias != nullptr) && !partial;
    float* yout = partial ? a.part : z.y;
    const int act = partial ? 0 : a.act;
    float* zout = act ? sel4(group, a.z0, a.z1, a.z2, a.z3) : nullptr;
    float aslope = a.slope;
    if (act == 1) aslope = *sel4(group, a.al0, a.al1, a.al2, a.al3);
    const bool stats = a.stats != nullptr && !partial;
    float bj[NI], s1[NI], s2[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = n0 + wn0 + j * 32 + l31;
        bj[j] = (add_bias && n < g.Cout) ? gbias[n] : 0.f;
        s1[j] = 0.f; s2[j] = 0.f;
    }
    {
        // lean path: full tile, consecutive output rows, byte offsets inside the 2 GB a buffer descriptor spans
        if (PM && !partial) {
            // position-major tile: 64 images at one pixel - the accumulator rows are an image apart (host: full tiles, < 2 GB)
            const int hwc = g.Hg * g.Wg * g.Cout;
            const unsigned vo = ((unsigned)((m0 & (g.pmn - 1)) + wm0 + 4 * h) * (unsigned)hwc + (unsigned)(pos_u * g.Cout + n0 + wn0 + l31)) * 4u;
            if (act) nn_store_lean<MI, NI, true>(acc, bj, yout, zout, vo, hwc * 4, act, aslope);
            else nn_store_lean<MI, NI, false>(acc, bj, yout, nullptr, vo, hwc * 4, 0, 0.f);
            CG_STAMP(3);
            return;
        }
        const bool lin = partial || (g.so == 1 && g.nphase == 1);
        const long rows_total = partial ? (long)a.nsplit * a.ngroups * g.nphase * g.M : (long)g.M;
        if (lin && !stats && m0 + BM <= g.M && n0 + BN <= g.Cout && rows_total * g.Cout < 0x1fffffffL) {
            const long rowbase = partial ? (long)(split * (a.ngroups * g.nphase) + zz) * g.M : 0L;
            const unsigned vo = ((unsigned)(rowbase + m0 + wm0 + 4 * h) * (unsigned)g.Cout + (unsigned)(n0 + wn0 + l31)) * 4u;
            if (act) nn_store_lean<MI, NI, true>(acc, bj, yout, zout, vo, g.Cout * 4, act, aslope);
            else nn_store_lean<MI, NI, false>(acc, bj, yout, nullptr, vo, g.Cout * 4, 0, 0.f);
            CG_STAMP(3);
            return;
        }
        // lean STRIDED path (round 5): the phase-folded forward of a layer behind an upsampling (output pixel (2 oy + a, 2 ox + b), so == 2)
        // with or without the batch-norm statistics of the layer behind it - power-of-two grids, full tiles, no fused activation, an
        // output below 2 GB: the pixel decode is shifts and masks, the byte offset of an accumulator row one 32-bit value, a row past
        // the end stores to the out-of-range offset.  (The generic loop below decodes, bounds-checks and builds a 64-bit address per
        // VALUE.)  Same values, same order of the statistics' sums.
        if constexpr (STRIDED) {
        if (!partial && !act && g.lgW >= 0 && m0 + BM <= g.M && n0 + BN <= g.Cout && !lin &&
            (long)(g.M >> g.lgHW) * g.Hout * g.Wout * g.Cout * 4L < 0x7fffffffL) {
            const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)yout, 0, 0x7fffffff, 0x00020000);
            const int colb = (n0 + wn0 + l31) * 4;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int n = m >> g.lgHW, oy = (m >> g.lgW) & (g.Hg - 1), ox = m & (g.Wg - 1);
                    const int vo = ((n * g.Hout + oy * g.so + pa) * g.Wout + ox * g.so + pb) * g.Cout * 4 + colb;
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        const float v = acc[i][j][r] + bj[j];
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ry, vo, j * 128, 0);
                        if (stats) { s1[j] += v; s2[j] = __builtin_fmaf(v, v, s2[j]); }
                    }
                }
            }
            if (stats) nn_store_stats<BM, WM, WN, NI, false>(a, s1, s2, zz, tm, wave, n0 + wn0 + l31, h);
            CG_STAMP(3);
            return;
        }
        }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= g.M) continue;
            const long ro = partial ? ((long)(split * (a.ngroups * g.nphase) + zz) * g.M + m) * g.Cout : out_row(g, m, pa, pb);
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int n = n0 + wn0 + j * 32 + l31;
                if (n < g.Cout) {
                    const float v = acc[i][j][r] + bj[j];
                    yout[ro + n] = v;
                    if (act) zout[ro + n] = cg::act(act, v, aslope);
                    if (stats) { s1[j] += v; s2[j] = NI == 1 ? __builtin_fmaf(v, v, s2[j]) : s2[j] + v * v; }
                }
            }
        }
    }
    if (stats) nn_store_stats<BM, WM, WN, NI, true>(a, s1, s2, zz, tm, wave, n0 + wn0 + l31, h);
    CG_STAMP(3);
}

// ---------------------------------------------------------------------------
// NN: Y[m][n] = sum_k A(m,k) * W[k][n]
// ---------------------------------------------------------------------------
//
template <int BM, int BN, int WM, int WN, bool FAST, bool VECB, int BK>
__global__ __launch_bounds__(256, BK == 16 ? 4 : 2) void igemm_nn_kernel(NNArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int MI = BM / WM / 32;
    constexpr int NI = BN / WN / 32;
    static_assert(MI >= 1 && NI >= 1, "wave tile >= 32x32");
    // A tile [k][m], column XOR-swizzled by ((k>>2)&3)<<3: the transposed ds_write_b32 of a float4 (4
    // consecutive k of one pixel) hits 32 distinct banks per half-wave, and a fragment read (32 consecutive m
    // at fixed k) stays a permutation of the 32 banks.  No padding.
    constexpr int LDA = BM, LDB = BN;
    constexpr int A_TILE = BK * LDA, B_TILE = BK * LDB;
    using Gather = NNGather<BM, BN, BK, false>;
    constexpr int KV = Gather::KV, ARPP = Gather::ARPP, AROWS = Gather::AROWS;       // float4 per A row, A rows per pass, float4 per thread per tile
    constexpr int NVEC = Gather::NVEC, BRPP = Gather::BRPP, BPASS = Gather::BPASS;   // B rows per pass

    __shared__ __attribute__((aligned(16))) float smem[2 * A_TILE + 2 * B_TILE];
    float* As = smem;
    float* Bs = smem + 2 * A_TILE;

    CG_STAMP(0);
    const Geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave / WN) * (BM / WM);
    const int wn0 = (wave % WN) * (BN / WN);

    const TileIdx ti = nn_tile_order<false, false>((g.Cout + BN - 1) / BN, a.xcd_swizzle);
    const int tm = ti.tm, split = ti.split;
    const int m0 = tm * BM, n0 = ti.tn * BN;
    const int zz = blockIdx.z;
    const NNTile z = nn_tile(a, zz);
    const int pa = z.pa, pb = z.pb;
    const float* gx = z.x;
    const float* wph = z.w;
    const int ks = split * a.kchunk;
    const int kend = min(g.Ktot, ks + a.kchunk);
    int T = CG_PROBE_HALF(1, (kend - ks + BK - 1) / BK);

    // ---- A staging: thread owns k-vector a_kv (4 consecutive k) of rows a_r + 64p
    const int a_kv = tid % KV, a_r = tid / KV;
    int rowb[AROWS], r_oy[AROWS], r_ox[AROWS];
    bool r_ok[AROWS];
#pragma unroll
    for (int p = 0; p < AROWS; ++p) Gather::decode_row(g, m0 + a_r + ARPP * p, 0, rowb[p], r_oy[p], r_ox[p], r_ok[p]);
    const int b_nv = tid % NVEC, b_kr = tid / NVEC;

    float4 areg[AROWS];
    float4 breg[BPASS];

    Gather gs;     // FAST-path state
    if (FAST) gs.start(g, z, gx, wph, a.kchunk, ks, split, T, a_kv, n0, b_nv, b_kr, rowb, r_oy, r_ox, r_ok);

    auto load_tile = [&](int k0) {
        if (FAST) {
            const int soff = gs.soff();
#pragma unroll
            for (int p = 0; p < AROWS; ++p) areg[p] = bufld4(gs.rsx, gs.avoff(p), soff);
            if (VECB) {
                const int sb = k0 * g.Cout * 4;
#pragma unroll
                for (int q = 0; q < BPASS; ++q) breg[q] = bufld4(gs.rsw, gs.bvoff[q], sb);
            }
            gs.advance(g, pa, pb);
        } else {
            float tmp[AROWS][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kj = k0 + 4 * a_kv + j;
                const bool kok = kj < kend;
                const int tap = kok ? kj / g.Cin : 0;
                const int ci = kj - tap * g.Cin;
                int ty, tx, off;
                tap_decode(g, tap, pa, pb, ty, tx, off);
#pragma unroll
                for (int p = 0; p < AROWS; ++p) {
                    const bool ok = r_ok[p] && kok && (unsigned)(r_oy[p] + ty) < (unsigned)g.Hv &&
                                    (unsigned)(r_ox[p] + tx) < (unsigned)g.Wv;
                    float v = 0.f;
                    if (ok) v = gx[(long)rowb[p] + off + ci];
                    tmp[p][j] = v;
                }
            }
#pragma unroll
            for (int p = 0; p < AROWS; ++p) areg[p] = make_float4(tmp[p][0], tmp[p][1], tmp[p][2], tmp[p][3]);
        }
        if (!(FAST && VECB)) {
#pragma unroll
            for (int q = 0; q < BPASS; ++q) {
                const int kr = b_kr + q * BRPP;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kr < BK) {
                    const int kk = k0 + kr;
                    const int n = n0 + 4 * b_nv;
                    if (kk < kend) {
                        const float* wp = wph + (long)kk * g.Cout + n;
                        if (VECB) {
                            if (n < g.Cout) v = ld4(wp);
                        } else {
                            if (n + 0 < g.Cout) v.x = wp[0];
                            if (n + 1 < g.Cout) v.y = wp[1];
                            if (n + 2 < g.Cout) v.z = wp[2];
                            if (n + 3 < g.Cout) v.w = wp[3];
                        }
                    }
                }
                breg[q] = v;
            }
        }
    };

    auto store_tile = [&](auto bufc) {   // compile-time buffer index: k_loop2
        constexpr int buf = decltype(bufc)::value;
        float* A = As + buf * A_TILE;
        float* B = Bs + buf * B_TILE;
#pragma unroll
        for (int p = 0; p < AROWS; ++p) {
            const int rs = (a_r + ARPP * p) ^ a_swizzle<BK>(a_kv);
            A[(4 * a_kv + 0) * LDA + rs] = areg[p].x;
            A[(4 * a_kv + 1) * LDA + rs] = areg[p].y;
            A[(4 * a_kv + 2) * LDA + rs] = areg[p].z;
            A[(4 * a_kv + 3) * LDA + rs] = areg[p].w;
        }
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int kr = b_kr + q * BRPP;
            if (kr < BK) *reinterpret_cast<float4*>(B + kr * LDB + 4 * b_nv) = breg[q];
        }
    };

    f32x16 acc[MI][NI] = {};

    CG_STAMP(6);   // trace builds: end of the integer set-up (tile origin, tap-validity masks, descriptors)
    if (T > 0) {
        load_tile(ks);
        store_tile(std::integral_constant<int, 0>{});
    }
    __syncthreads();
    CG_STAMP(1);

    auto k_tile = [&](auto bufc, int t) {
        constexpr int buf = decltype(bufc)::value;
        if (t + 1 < T) load_tile(ks + (t + 1) * BK);   // tile t + 1 into the staging registers, stored to LDS behind this tile's MFMAs
        mfma_k_major<MI, NI, LDA, LDB, BK, true>(acc, As + buf * A_TILE + wm0, Bs + buf * B_TILE + wn0 + l31, h, l31);
        if (t + 1 < T) store_tile(std::integral_constant<int, buf ^ 1>{});
        __syncthreads();
    };
    // (k_loop2's loop, spelled out: through the shared driver this kernel's short launches - nn.Linear 100 -> 8192 forward, 7 K tiles - ran
    // 17.8 us against the parent's 17.5 in every alternating run, with the same instructions in the loop, and no other form of the driver
    // brought them back: profiles/gemm_prologue_refactor.txt, section 3)
    for (int t = 0; t < T; t += 2) {
        k_tile(std::integral_constant<int, 0>{}, t);
        if (t + 1 < T) k_tile(std::integral_constant<int, 1>{}, t + 1);
    }

    CG_STAMP(2);
    nn_epilogue<BM, BN, WM, WN, false, false>(acc, a, z, m0, n0, wm0, wn0, l31, h, wave, tm, zz, split, 0);
}

// ---------------------------------------------------------------------------
// NN with LDS-direct loads (buffer_load_dwordx4 ... lds, gfx950): the tiles go from global memory straight into LDS - no
// staging registers, no ds_write, no wait for a load in front of a store.  (Ablation of igemm_nn_kernel, CG_EXP builds: the
// K loop of the 512 -> 256 data gradient runs 0.318 ms; without its LDS stores and the loads feeding them 0.271 ms.)
// A lane's 16 bytes land at M0 + 16 * lane, so a wave instruction fills 1 KB of consecutive LDS and the tile layouts follow
// from which global quad every lane asks for:
//   A: row-major [m][BK] (a pixel's BK consecutive channels = 8 or 4 quads); the lane at position (m, j) loads quad
//      j ^ swz(m), swz(m) = (m >> 1) & 7 (BK 32) / (m >> 2) & 3 (BK 16), so that a ds_read_b128 fragment read (16 lanes = 16
//      rows, one quad each) covers all 16 bank slots while 8 (4) neighbouring lanes still fetch one pixel's 128 (64)
//      consecutive bytes.  A lane whose tap falls into the padding asks for the out-of-range offset and its quad is
//      written as zeros (checked on the hardware: tools/glds_test.hip).
//   B: [k][n] as in igemm_nn_kernel (a wave instruction = 64 / (BN/4) consecutive weight rows), ds_read_b32 fragments.
// MFMA step (g, s) multiplies A[m][8g + 4h + s] with B[8g + 4h + s][n] (h = lane / 32).
// FAST && VECB geometries only (Cin % BK == 0, 16-byte aligned operands, Cout % 4 == 0); prologue and epilogue as above.
// ---------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int BK, bool PM = false>
__global__ __launch_bounds__(256, 2) void igemm_nng_kernel(NNArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int MI = BM / WM / 32;
    constexpr int NI = BN / WN / 32;
    constexpr int A_TILE = BK * BM, B_TILE = BK * BN;
    using Gather = NNGather<BM, BN, BK, PM>;
    constexpr int KV = Gather::KV, ARPP = Gather::ARPP, AROWS = Gather::AROWS;       // quads per A row, A rows per pass of the workgroup
    constexpr int NVEC = Gather::NVEC, BRPP = Gather::BRPP, BPASS = Gather::BPASS;   // B rows per pass
    constexpr int RPW = 64 / KV;      // A rows per wave instruction
    constexpr int BRPW = 64 / NVEC;   // B rows per wave instruction
    constexpr int G2 = KV / 2;

    // separate arrays per buffer: the compiler can then tell the buffer the DMA writes from the one the fragments are read from
    __shared__ __attribute__((aligned(16))) float As0[A_TILE];
    __shared__ __attribute__((aligned(16))) float As1[A_TILE];
    __shared__ __attribute__((aligned(16))) float Bs0[B_TILE];
    __shared__ __attribute__((aligned(16))) float Bs1[B_TILE];

    CG_STAMP(0);
    const Geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave / WN) * (BM / WM);
    const int wn0 = (wave % WN) * (BN / WN);

    const TileIdx ti = nn_tile_order<true, PM>((g.Cout + BN - 1) / BN, a.xcd_swizzle);
    const int tm = ti.tm, split = ti.split;
    const int m0 = tm * BM, n0 = ti.tn * BN;
    const int zz = blockIdx.z;
    const NNTile z = nn_tile(a, zz);
    const int pa = z.pa, pb = z.pb;
    const float* gx = z.x;
    const float* wph = z.w;
    const int ks = split * a.kchunk;
    const int kend = min(g.Ktot, ks + a.kchunk);
    int T = (kend - ks + BK - 1) / BK;
    const int pos_u = PM ? (m0 >> g.pm_lg) : 0;      // PM: the tile's pixel position (wave-uniform; N is a multiple of BM)

    // ---- A: lane -> (row a_r + ARPP p, LDS quad position a_kv); the quad it loads is a_kv ^ swz(row)
    const int a_kv = tid % KV, a_r = tid / KV;
    const int a_sw = KV == 8 ? ((a_r >> 1) & 7) : ((a_r >> 2) & 3);   // ARPP is a multiple of 16: the same for every pass
    int rowb[AROWS], r_oy[AROWS], r_ox[AROWS];
    bool r_ok[AROWS];
#pragma unroll
    for (int p = 0; p < AROWS; ++p) Gather::decode_row(g, m0 + a_r + ARPP * p, pos_u, rowb[p], r_oy[p], r_ox[p], r_ok[p]);
    const int b_nv = tid % NVEC, b_kr = tid / NVEC;
    Gather gs;
    if (!gs.start(g, z, gx, wph, a.kchunk, ks, split, T, a_kv ^ a_sw, n0, b_nv, b_kr, rowb, r_oy, r_ox, r_ok)) return;

    // request tile k0 (the FAST-path state describes it) into buffer `buf`; the wave's own 1 KB pieces
    auto dma_tile = [&](int k0, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        float* A = buf ? As1 : As0;
        float* B = buf ? Bs1 : Bs0;
        const int soff = gs.soff();
        if (PM) k0 = gs.tapi * g.Cin + gs.ci0;       // the weight rows of the tap the walk is at
#pragma unroll
        for (int p = 0; p < AROWS; ++p) glds16(gs.rsx, A + (ARPP * p + wave * RPW) * BK, gs.avoff(p), soff);
        const int sb = k0 * g.Cout * 4;
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int row0 = q * BRPP + wave * BRPW;   // wave-uniform
            if (BPASS * BRPP == BK || row0 < BK)
                glds16(gs.rsw, B + row0 * BN, gs.bvoff[q], sb);
        }
        gs.advance(g, pa, pb);
    };

    f32x16 acc[MI][NI] = {};

    T = CG_PROBE_HALF(1, T);
    if (T > 0) dma_tile(ks, std::integral_constant<int, 0>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CG_STAMP(1);

    // fragment addresses: A quad (row, kq) at float4 index row * KV + (kq ^ swz(row)); swz depends on l31 only
    const int f_sw = KV == 8 ? ((l31 >> 1) & 7) : ((l31 >> 2) & 3);
    int qa_rd[G2];
#pragma unroll
    for (int gq = 0; gq < G2; ++gq) qa_rd[gq] = (wm0 + l31) * KV + ((2 * gq + h) ^ f_sw);
    const int qb_rd = 4 * h * BN + wn0 + l31;

    auto k_tile = [&](auto bufc, int t) {
        constexpr int buf = decltype(bufc)::value;
        if (t + 1 < T) dma_tile(ks + (t + 1) * BK, std::integral_constant<int, buf ^ 1>{});
        const float4* A4 = reinterpret_cast<const float4*>(buf ? As1 : As0);
        const float* B = (buf ? Bs1 : Bs0) + qb_rd;
#pragma unroll
        for (int gq = 0; gq < G2; ++gq) {
            float4 af[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = A4[qa_rd[gq] + i * 32 * KV];
#pragma unroll
            for (int sidx = 0; sidx < 4; ++sidx) {
                float bv[NI];
#pragma unroll
                for (int j = 0; j < NI; ++j) bv[j] = B[(8 * gq + sidx) * BN + j * 32];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(af[i], sidx), bv[j], acc[i][j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile t + 1 are in LDS
        __syncthreads();
    };
    k_loop2(T, k_tile);

    CG_STAMP(2);
    nn_epilogue<BM, BN, WM, WN, true, PM>(acc, a, z, m0, n0, wm0, wn0, l31, h, wave, tm, zz, split, pos_u);
}

// split-K reduce for NN: y_group[out_row(m)][n] = bias_group[n] + sum_s part[s][group*nphase+phase][m][n]
// LANES > 1: 256/LANES outputs per workgroup, the S partials of one output shared by LANES threads (small outputs
// with many splits would otherwise be one long serial load chain per thread).
template <int LANES, bool V4 = false>
__global__ __launch_bounds__(256) void nn_splitk_reduce_kernel(NNArgs a, int S) {
    constexpr int OUTS = 256 / LANES;
    __shared__ float sh[LANES > 1 ? LANES : 1][OUTS + 1];
    const Geom& g = a.g;
    const long PMN = (long)a.ngroups * g.nphase * g.M * g.Cout;
    if (LANES == 1 && V4) {
        // four consecutive channels of one output row per thread (host: Cout % 4 == 0, 16-byte aligned tensors): 16-byte loads, four
        // partial planes in flight, each element's splits still added in order 0 .. S-1 - the same bits as the scalar form below,
        // which moved 12 MB in 41 us beside the other queue's GEMMs (round 5)
        const long PMN4 = PMN >> 2;
        const int C4 = g.Cout >> 2;
        const float4* part4 = reinterpret_cast<const float4*>(a.part);
        for (long i4 = blockIdx.x * 256L + threadIdx.x; i4 < PMN4; i4 += (long)gridDim.x * 256) {
            const int n = (int)(i4 % C4) * 4;
            const long pm = i4 / C4;
            const int m = (int)(pm % g.M);
            const int zz = (int)(pm / g.M);
            int Se = S;
            if (g.pmn) Se = (pm_valid_taps(g, m >> g.pm_lg) * g.Cin + a.kchunk - 1) / a.kchunk;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            int k = 0;
            for (; k + 4 <= Se; k += 4) {
                const float4 p0 = part4[(long)k * PMN4 + i4], p1 = part4[(long)(k + 1) * PMN4 + i4];
                const float4 p2 = part4[(long)(k + 2) * PMN4 + i4], p3 = part4[(long)(k + 3) * PMN4 + i4];
                s.x += p0.x; s.y += p0.y; s.z += p0.z; s.w += p0.w;
                s.x += p1.x; s.y += p1.y; s.z += p1.z; s.w += p1.w;
                s.x += p2.x; s.y += p2.y; s.z += p2.z; s.w += p2.w;
                s.x += p3.x; s.y += p3.y; s.z += p3.z; s.w += p3.w;
            }
            for (; k < Se; ++k) {
                const float4 p0 = part4[(long)k * PMN4 + i4];
                s.x += p0.x; s.y += p0.y; s.z += p0.z; s.w += p0.w;
            }
            const int group = zz / g.nphase, phase = zz - group * g.nphase;
            const float* gbias = sel4(group, a.b0, a.b1, a.b2, a.b3);
            float* gy = sel4(group, a.y0, a.y1, a.y2, a.y3);
            if (gbias) { const float4 b = ld4(gbias + n); s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w; }
            const long o = out_row(g, m, phase >> 1, phase & 1) + n;
            *reinterpret_cast<float4*>(gy + o) = s;
            if (a.act) {
                const float al = a.act == 1 ? *sel4(group, a.al0, a.al1, a.al2, a.al3) : a.slope;
                *reinterpret_cast<float4*>(sel4(group, a.z0, a.z1, a.z2, a.z3) + o) =
                    make_float4(cg::act(a.act, s.x, al), cg::act(a.act, s.y, al), cg::act(a.act, s.z, al), cg::act(a.act, s.w, al));
            }
        }
        return;
    }
    const int ol = threadIdx.x % OUTS, ln = threadIdx.x / OUTS;
    for (long i0 = blockIdx.x * (long)OUTS; i0 < PMN; i0 += (long)gridDim.x * OUTS) {
        const long i = i0 + ol;
        float s = 0.f;
        if (i < PMN) {
            int Se = S;
            if (g.pmn) Se = (pm_valid_taps(g, (int)((i / g.Cout) % g.M) >> g.pm_lg) * g.Cin + a.kchunk - 1) / a.kchunk;   // this pixel's K units
            for (int k = ln; k < Se; k += LANES) s += a.part[(long)k * PMN + i];
        }
        if (LANES > 1) {
            __syncthreads();
            sh[ln][ol] = s;
            __syncthreads();
            if (ln != 0) continue;
            s = 0.f;
#pragma unroll
            for (int r = 0; r < LANES; ++r) s += sh[r][ol];
        }
        if (i >= PMN) continue;
        const int n = (int)(i % g.Cout);
        const long pm = i / g.Cout;
        const int m = (int)(pm % g.M);
        const int zz = (int)(pm / g.M);
        const int group = zz / g.nphase, phase = zz - group * g.nphase;
        const float* gbias = sel4(group, a.b0, a.b1, a.b2, a.b3);
        float* gy = sel4(group, a.y0, a.y1, a.y2, a.y3);
        if (gbias) s += gbias[n];
        const long o = out_row(g, m, phase >> 1, phase & 1) + n;
        gy[o] = s;
        if (a.act) {
            const float al = a.act == 1 ? *sel4(group, a.al0, a.al1, a.al2, a.al3) : a.slope;
            sel4(group, a.z0, a.z1, a.z2, a.z3)[o] = cg::act(a.act, s, al);
        }
    }
}

// the (split, group, phase) plane of a weight-gradient launch's partials: part[plane][Ktot][Cout] (tn_part), bias_part[plane][Cout]
__device__ __forceinline__ long tn_plane(const TNArgs& a, int split, int zz) { return (long)(split * (a.ngroups * a.g.nphase) + zz); }
__device__ __forceinline__ float* tn_part(const TNArgs& a, int split, int zz) { return a.part + tn_plane(a, split, zz) * a.g.Ktot * a.g.Cout; }

// generic tail of both TN kernels: the bounds-checked store of a wave's accumulators into its plane of the partials
template <int MI, int NI>
__device__ __forceinline__ void tn_store_partials(const f32x16 (&acc)[MI][NI], float* pout, const Geom& g, int m0, int n0, int wm0, int wn0, int l31,
                                                  int h) {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = n0 + wn0 + j * 32 + l31;
        if (n >= g.Cout) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < g.Ktot) pout[(long)m * g.Cout + n] = acc[i][j][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// TN: dW[k][n] = sum_m A(m,k) * dY[m][n]   (k = (tap,ci) rows, m = grid pixels reduced)
// ---------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool VECA, bool VECB>
__global__ __launch_bounds__(256, 4) void igemm_tn_kernel(TNArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int MI = BM / WM / 32;
    constexpr int NI = BN / WN / 32;
    constexpr int LDA = BM, LDB = BN;
    constexpr int A_TILE = BK * LDA, B_TILE = BK * LDB;
    constexpr int AVEC = BM / 4, ARPP = 256 / AVEC, APASS = (BK + ARPP - 1) / ARPP;
    constexpr int BVEC = BN / 4, BRPP = 256 / BVEC, BPASS = (BK + BRPP - 1) / BRPP;
    constexpr int NJ = VECA ? 1 : 4;

    __shared__ __attribute__((aligned(16))) float smem[2 * A_TILE + 2 * B_TILE];
    float* As = smem;
    float* Bs = smem + 2 * A_TILE;

    const Geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave / WN) * (BM / WM);
    const int wn0 = (wave % WN) * (BN / WN);

    const TileIdx ti = tn_tile_order((g.Cout + BN - 1) / BN, a.xcd_swizzle);
    const int tm = ti.tm, tn = ti.tn, split = ti.split;
    const int m0 = tm * BM, n0 = tn * BN;  // m0: row of dW (tap,ci)
    const int zz = blockIdx.z;
    const TNTile z = tn_tile(a, zz);
    const int pa = z.pa, pb = z.pb;
    const float* gx = z.x;
    const float* gdy = z.dy;
    const int ps = split * a.pchunk;
    const int pend = min(g.M, ps + a.pchunk);
    const int T = CG_PROBE_HALF(2, (pend - ps + BK - 1) / BK);

    // A staging: fixed (tap,ci) columns per thread, pixel rows vary per tile
    const int a_mv = tid % AVEC, a_kr = tid / AVEC;
    int c_off[NJ], c_ty[NJ], c_tx[NJ];
    bool c_ok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) tn_col_decode(g, m0 + 4 * a_mv + j, pa, pb, c_ok[j], c_ty[j], c_tx[j], c_off[j]);
    const int b_nv = tid % BVEC, b_kr = tid / BVEC;
    const bool b_nok = n0 + 4 * b_nv < g.Cout;
    __amdgpu_buffer_rsrc_t rsx = buf_rsrc(gx);
    __amdgpu_buffer_rsrc_t rsd = buf_rsrc(gdy);

    float4 areg[APASS];
    float4 breg[BPASS];
    // gradBias rides along: the dW row-tile 0 of every column tile also sums the dy rows it streams
    const bool do_bias = a.bias_part != nullptr && tm == 0;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);

    // The generic gather below decodes the pixel once per row and shares it between both operands when their row mappings coincide; the
    // lean arm (tn_lean_geom; vector loads, whole K tiles, whole passes) keeps every per-tile VALU op out of the loop.
    const bool lin_src = tn_lin_src(g), lin_out = tn_lin_out(g);
    constexpr bool SAME_ROWS = (AVEC == BVEC);
    const bool lean = VECA && VECB && tn_lean_geom(g) && (ps % BK) == 0 && (pend % BK) == 0 && APASS * ARPP == BK && BPASS * BRPP == BK;
    int l_ay[APASS], l_ax[APASS];
    unsigned l_avoff[APASS], l_bvoff[BPASS];
    int l_minoff = 0;
    __amdgpu_buffer_rsrc_t rsx_l = rsx;
    if (lean) {
        l_minoff = sel4(z.phase, g.minoff0, g.minoff1, g.minoff2, g.minoff3);   // host-computed (finish_geom)
        rsx_l = buf_rsrc(gx + l_minoff);
        tn_lean_a<APASS, ARPP>(g, 0, a_kr, c_ok[0], c_ty[0], c_tx[0], c_off[0], l_minoff, l_ay, l_ax, l_avoff);
        tn_lean_b<BPASS, BRPP>(g, 0, b_kr, b_nok, n0, b_nv, l_bvoff);
    }
    auto load_tile = [&](int p0) {
        if (lean) {
            int oyb, oxb, soa, sob;
            tn_tile_bases(g, false, p0, pa, pb, oyb, oxb, soa, sob);
#pragma unroll
            for (int q = 0; q < APASS; ++q) areg[q] = bufld4(rsx_l, tn_row_ok(g, oyb + l_ay[q], oxb + l_ax[q]) ? l_avoff[q] : OOB, soa);
#pragma unroll
            for (int q = 0; q < BPASS; ++q) breg[q] = bufld4(rsd, l_bvoff[q], sob);
            return;
        }
        int rn[APASS], roy[APASS], rox[APASS];
#pragma unroll
        for (int q = 0; q < APASS; ++q) {
            const int kr = a_kr + q * ARPP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (APASS * ARPP == BK || kr < BK) {
                const int pix = p0 + kr;
                const bool pok = pix < pend;
                int n, oy, ox;
                pix_decode(g, pok ? pix : 0, n, oy, ox);
                rn[q] = n; roy[q] = oy; rox[q] = ox;
                const int base = lin_src ? pix * g.Cin : ((n * g.Hs + oy * g.td.ss) * g.Ws + ox * g.td.ss) * g.Cin;
                if (VECA) {
                    const bool ok = pok && c_ok[0] && (unsigned)(oy + c_ty[0]) < (unsigned)g.Hv &&
                                    (unsigned)(ox + c_tx[0]) < (unsigned)g.Wv;
                    v = bufld4(rsx, ok ? (unsigned)(base + c_off[0]) * 4u : OOB, 0);
                } else {
                    float t4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int jj = VECA ? 0 : j;
                        const bool ok = pok && c_ok[jj] && (unsigned)(oy + c_ty[jj]) < (unsigned)g.Hv &&
                                        (unsigned)(ox + c_tx[jj]) < (unsigned)g.Wv;
                        float e = 0.f;
                        if (ok) e = gx[(long)base + c_off[jj]];
                        t4[j] = e;
                    }
                    v = make_float4(t4[0], t4[1], t4[2], t4[3]);
                }
            }
            areg[q] = v;
        }
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int kr = b_kr + q * BRPP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BPASS * BRPP == BK || kr < BK) {
                const int pix = p0 + kr;
                const bool pok = pix < pend;
                const int n = n0 + 4 * b_nv;
                int ro;
                if (lin_out) {
                    ro = pix * g.Cout;
                } else {
                    int pn, poy, pox;
                    if (SAME_ROWS) { pn = rn[q < APASS ? q : 0]; poy = roy[q < APASS ? q : 0]; pox = rox[q < APASS ? q : 0]; }
                    else pix_decode(g, pok ? pix : 0, pn, poy, pox);
                    ro = ((pn * g.Hout + poy * g.so + pa) * g.Wout + pox * g.so + pb) * g.Cout;
                }
                if (VECB) {
                    v = bufld4(rsd, (pok && b_nok) ? (unsigned)(ro + n) * 4u : OOB, 0);
                } else if (pok) {
                    const float* dp = gdy + (long)ro + n;
                    if (n + 0 < g.Cout) v.x = dp[0];
                    if (n + 1 < g.Cout) v.y = dp[1];
                    if (n + 2 < g.Cout) v.z = dp[2];
                    if (n + 3 < g.Cout) v.w = dp[3];
                }
            }
            breg[q] = v;
        }
    };

    auto store_tile = [&](auto bufc) {   // compile-time buffer index: k_loop2
        constexpr int buf = decltype(bufc)::value;
        float* A = As + buf * A_TILE;
        float* B = Bs + buf * B_TILE;
#pragma unroll
        for (int q = 0; q < APASS; ++q) {
            const int kr = a_kr + q * ARPP;
            if (APASS * ARPP == BK || kr < BK) *reinterpret_cast<float4*>(A + kr * LDA + 4 * a_mv) = areg[q];
        }
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int kr = b_kr + q * BRPP;
            if (BPASS * BRPP == BK || kr < BK) {
                *reinterpret_cast<float4*>(B + kr * LDB + 4 * b_nv) = breg[q];
                if (do_bias) { bsum.x += breg[q].x; bsum.y += breg[q].y; bsum.z += breg[q].z; bsum.w += breg[q].w; }
            }
        }
    };

    f32x16 acc[MI][NI] = {};

    if (T > 0) {
        load_tile(ps);
        store_tile(std::integral_constant<int, 0>{});
    }
    __syncthreads();

    auto k_tile = [&](auto bufc, int t) {
        constexpr int buf = decltype(bufc)::value;
        if (t + 1 < T) load_tile(ps + (t + 1) * BK);
        const float* A = As + buf * A_TILE + wm0 + l31;
        const float* B = Bs + buf * B_TILE + wn0 + l31;
        mfma_k_major<MI, NI, LDA, LDB, BK, false>(acc, A, B, h, l31);
        if (t + 1 < T) store_tile(std::integral_constant<int, buf ^ 1>{});
        __syncthreads();
    };
    k_loop2(T, k_tile);

    if (do_bias) {  // all waves are past the loop's final barrier: reuse the A tile as scratch
        float* red = smem;
        *reinterpret_cast<float4*>(red + b_kr * BN + 4 * b_nv) = bsum;
        __syncthreads();
        if (tid < BN && n0 + tid < g.Cout) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < 256 / BVEC; ++r) t += red[r * BN + tid];
            a.bias_part[tn_plane(a, split, zz) * g.Cout + n0 + tid] = t;
        }
    }
    tn_store_partials<MI, NI>(acc, tn_part(a, split, zz), g, m0, n0, wm0, wn0, l31, h);
}

// ---------------------------------------------------------------------------
// TN with LDS-direct loads (see igemm_nng_kernel): both operands are pixel rows of consecutive channels, i.e. already the
// K-major [pixel][column] tiles the MFMA fragments are read from, so a wave instruction simply drops 64 / (BM / 4) pixel
// rows of 4 BM bytes into place (no swizzle, ds_read_b32 fragments exactly as in igemm_tn_kernel).  Lean addressing only
// (the host checks, tng_ok): 16-byte aligned channel quads, a source tensor with the grid's geometry, a reduction range of whole K
// tiles, and either a power-of-two grid with HWg >= 16 (a K tile never straddles two images) or a 1 x 1 kernel without padding
// (`flat`, mode 1: every row is valid and rows are simply consecutive - the linear layers and the Winograd-domain GEMMs).
//
// Mode 2, POSITION-MAJOR K tiles (round 6; models.lua:681,685 - D32_st3's 5x5 and 7x7 layers - and :696-697, the View -> Linear head as
// an H x W convolution): a K tile is ONE grid position (oy, ox) of 16 consecutive images, so all its rows share their zero-padding taps
// and a workgroup - whose dW rows belong to one or two taps - runs its K loop only over the rectangle of positions at which one of its
// taps reads inside the image: the 38 % / 14 % of the MACs that multiply padding are not issued.  The splits divide each workgroup's
// OWN tile list evenly, rows of a tile are a whole image apart (a per-lane offset, as before), and the grid needs no power-of-two
// geometry, nor 16 pixels per image.  gradBias rides on the row tile that holds the centre tap (its rectangle is the whole grid).
// ---------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void igemm_tng_kernel(TNArgs a, int mode) {
    const int flat = mode == 1;
    const bool pm = mode == 2;
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int MI = BM / WM / 32;
    constexpr int NI = BN / WN / 32;
    constexpr int LDA = BM, LDB = BN;
    constexpr int A_TILE = BK * LDA, B_TILE = BK * LDB;
    constexpr int AVEC = BM / 4, ARPP = 256 / AVEC, APASS = (BK + ARPP - 1) / ARPP, ARPW = 64 / AVEC;
    constexpr int BVEC = BN / 4, BRPP = 256 / BVEC, BPASS = (BK + BRPP - 1) / BRPP, BRPW = 64 / BVEC;

    __shared__ __attribute__((aligned(16))) float As0[A_TILE];
    __shared__ __attribute__((aligned(16))) float As1[A_TILE];
    __shared__ __attribute__((aligned(16))) float Bs0[B_TILE];
    __shared__ __attribute__((aligned(16))) float Bs1[B_TILE];

    const Geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    // (Round 5 tried INTERLEAVING a wave's 32-row blocks with the other waves' - 64 floats apart, so that a fragment pair is one
    // ds_read2st64_b32 with immediate offsets and the K loop has no address VALU at all (the ds_read2_b32 pairs below need one v_add_u32
    // per pair: their 8-bit offsets reach 1 KB).  Alone the weight gradients measured the same; in the step it cost 0.12 ms
    // (6.00 against 5.88 ms, profiles/r05_sweeps.txt) - the two reads of a pair then hit the same LDS banks.  Not kept.)
    const int wm0 = (wave / WN) * (BM / WM);
    const int wn0 = (wave % WN) * (BN / WN);

    const TileIdx ti = tn_tile_order((g.Cout + BN - 1) / BN, a.xcd_swizzle);
    const int tm = ti.tm, tn = ti.tn, split = ti.split;
    const int m0 = tm * BM, n0 = tn * BN;
    const int zz = blockIdx.z;
    const TNTile z = tn_tile(a, zz);
    const int pa = z.pa, pb = z.pb;
    const float* gx = z.x;
    const float* gdy = z.dy;
    const int ps = split * a.pchunk;
    const int pend = min(g.M, ps + a.pchunk);
    int T = CG_PROBE_HALF(2, (pend - ps) / BK);
    int q_c = 0, q_x = 0, q_y = 0, q_x0 = 0, q_x1 = 0, q_nc = 1;   // mode 2: image chunk / position of the next tile, the rectangle's columns
    if (pm) {
        const int t_lo = m0 / g.Cin, t_hi = min(g.Ktot - 1, m0 + BM - 1) / g.Cin;
        int y0 = g.Hg, y1 = 0, x0 = g.Wg, x1 = 0;
        for (int t = t_lo; t <= t_hi; ++t) {
            int ty, tx, off;
            tap_decode(g, t, pa, pb, ty, tx, off);
            y0 = min(y0, max(0, -ty)); y1 = max(y1, min(g.Hg, g.Hv - ty));
            x0 = min(x0, max(0, -tx)); x1 = max(x1, min(g.Wg, g.Wv - tx));
        }
        const int rw = max(0, x1 - x0), rh = max(0, y1 - y0);
        q_nc = a.pm_n / BK;
        const long L = (long)rw * rh * q_nc;
        const int u0 = (int)(L * split / (int)gridDim.y), u1 = (int)(L * (split + 1) / (int)gridDim.y);
        T = CG_PROBE_HALF(2, u1 - u0);
        if (T > 0) {
            const int pos = u0 / q_nc;
            q_c = u0 - pos * q_nc;
            q_y = y0 + pos / rw; q_x = x0 + pos % rw;
        }
        q_x0 = x0; q_x1 = x1;
    }

    const int a_mv = tid % AVEC, a_kr = tid / AVEC;
    const int b_nv = tid % BVEC, b_kr = tid / BVEC;
    int c_ty, c_tx, c_off;
    bool c_ok;
    tn_col_decode(g, m0 + 4 * a_mv, pa, pb, c_ok, c_ty, c_tx, c_off);
    const int l_minoff = sel4(z.phase, g.minoff0, g.minoff1, g.minoff2, g.minoff3);   // host-computed (finish_geom)
    __amdgpu_buffer_rsrc_t rsx = buf_rsrc(gx + l_minoff);
    __amdgpu_buffer_rsrc_t rsd = buf_rsrc(gdy);
    int l_ay[APASS], l_ax[APASS];
    unsigned l_avoff[APASS], l_bvoff[BPASS];
    tn_lean_a<APASS, ARPP>(g, mode, a_kr, c_ok, c_ty, c_tx, c_off, l_minoff, l_ay, l_ax, l_avoff);
    tn_lean_b<BPASS, BRPP>(g, mode, b_kr, n0 + 4 * b_nv < g.Cout, n0, b_nv, l_bvoff);
    // gradBias rides along on the row-tile 0 workgroups (mode 2: the tile of the tap at offset (0, 0), which visits every position):
    // column sums of the dy rows, read back from the LDS tile
    const int tm_bias = pm ? ((-g.td.r0y0) * g.td.kw + (-g.td.r0x0)) * g.Cin / BM : 0;
    const bool do_bias = a.bias_part != nullptr && tm == tm_bias;
    float bsum = 0.f;

    auto dma_tile = [&](int p0, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        float* A = buf ? As1 : As0;
        float* B = buf ? Bs1 : Bs0;
        int oyb, oxb, soa, sob;
        if (pm) {   // wave-uniform: the next tile of this workgroup's list
            oyb = q_y; oxb = q_x;
            soa = ((q_c * BK * g.Hs + q_y) * g.Ws + q_x) * g.Cin * 4;
            sob = ((q_c * BK * g.Hout + q_y) * g.Wout + q_x) * g.Cout * 4;
            if (++q_c == q_nc) {
                q_c = 0;
                if (++q_x == q_x1) { q_x = q_x0; ++q_y; }
            }
        } else tn_tile_bases(g, flat, p0, pa, pb, oyb, oxb, soa, sob);
#pragma unroll
        for (int q = 0; q < APASS; ++q) {
            const int row0 = q * ARPP + wave * ARPW;   // wave-uniform
            if (APASS * ARPP == BK || row0 < BK) glds16(rsx, A + row0 * LDA, tn_row_ok(g, oyb + l_ay[q], oxb + l_ax[q]) ? l_avoff[q] : OOB, soa);
        }
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int row0 = q * BRPP + wave * BRPW;
            if (BPASS * BRPP == BK || row0 < BK) glds16(rsd, B + row0 * LDB, l_bvoff[q], sob);
        }
    };

    f32x16 acc[MI][NI] = {};

    if (T > 0) dma_tile(ps, std::integral_constant<int, 0>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    auto k_tile = [&](auto bufc, int t) {
        constexpr int buf = decltype(bufc)::value;
        if (t + 1 < T) dma_tile(ps + (t + 1) * BK, std::integral_constant<int, buf ^ 1>{});
        const float* A = (buf ? As1 : As0) + wm0 + l31;
        const float* B = (buf ? Bs1 : Bs0) + wn0 + l31;
        if (do_bias && tid < BN) {
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) bsum += (buf ? Bs1 : Bs0)[kk * LDB + tid];
        }
        mfma_k_major<MI, NI, LDA, LDB, BK, false>(acc, A, B, h, l31);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    k_loop2(T, k_tile);

    if (do_bias && tid < BN && n0 + tid < g.Cout)
        a.bias_part[tn_plane(a, split, zz) * g.Cout + n0 + tid] = bsum;
    float* pout = tn_part(a, split, zz);
    // lean path (round 5, as nn_store_lean): a FULL tile stores through a buffer descriptor at (per-lane byte offset) + (row offset in an
    // SGPR) - no bounds test, no 64-bit address per value (the generic loop below is ~2000 instructions per wave, 1 VALU per MFMA of the
    // whole launch; the partial sums of one (split, phase) plane always fit the 2 GB a descriptor spans)
    if (m0 + BM <= g.Ktot && n0 + BN <= g.Cout && (long)g.Ktot * g.Cout * 4L < 0x7fffffffL) {
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)pout, 0, 0x7fffffff, 0x00020000);
        const unsigned vo = ((unsigned)(m0 + wm0 + 4 * h) * (unsigned)g.Cout + (unsigned)(n0 + wn0 + l31)) * 4u;
        const int c4 = g.Cout * 4;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int soff = (i * 32 + (r & 3) + 8 * (r >> 2)) * c4;   // wave-uniform
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[i][j][r]), rp, (int)(vo + j * 128), soff, 0);
            }
        return;
    }
    tn_store_partials<MI, NI>(acc, pout, g, m0, n0, wm0, wn0, l31, h);
}


// ---- host-side dispatch -----------------------------------------------------
struct TileCfg { int bm, bn; };
// the compiled block tiles (BM x BN, WM x WN waves) of all four GEMM kernels: launch(BlockTile<...>{}) for the one the plan chose
template <int BM_, int BN_, int WM_, int WN_> struct BlockTile { static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_; };
template <class Launch>
static void with_block_tile(const TileCfg& tc, Launch&& launch) {
    if (tc.bm == 128 && tc.bn == 128) launch(BlockTile<128, 128, 2, 2>{});
    else if (tc.bm == 64 && tc.bn == 128) launch(BlockTile<64, 128, 2, 2>{});
    else if (tc.bm == 128 && tc.bn == 64) launch(BlockTile<128, 64, 2, 2>{});
    else if (tc.bm == 64 && tc.bn == 64) launch(BlockTile<64, 64, 2, 2>{});
    else launch(BlockTile<128, 32, 4, 1>{});
}
// swept in rounds 2-5 (profiles/r0N_sweeps.txt: flat or worse around these), constants since round 6
constexpr int kSplitTarget = 1, kSplitMinK = 8;      // forward / data gradient: split K until one workgroup per CU, >= 8 K iterations per split
constexpr int kTnSplitMax = 256, kTnTarget = 3;      // weight gradients: pixel splits up to 256, three workgroups per CU

// pick the block tile: BN covers Cout with least padding, BM chosen so the grid
// fills the 256 CUs at >= ~2 workgroups each when the problem allows it.
static bool tile_forced(cg::Opt o, TileCfg& tc) {
    // CG_NN_TILE / CG_TN_TILE = bm*1000 + bn forces one of the compiled block tiles (parity tests walk all of them)
    const long v = cg::opt(o);
    if (v <= 0) return false;
    const int bm = (int)(v / 1000), bn = (int)(v % 1000);
    if (!((bm == 128 || bm == 64) && (bn == 128 || bn == 64)) && !(bm == 128 && bn == 32)) return false;
    tc = {bm, bn};
    return true;
}

static TileCfg pick_tile(long M, int Cout, int nphase) {
    TileCfg f;
    if (tile_forced(cg::OPT_NN_TILE, f)) return f;
    int bn = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
    int bm = 128;
    if (bn == 128 || bn == 64) {
        const long blocks128 = ((M + 127) / 128) * ((Cout + bn - 1) / bn) * nphase;
        if (blocks128 < 2 * cg::kNumCU) bm = 64;   // swept 256 .. 2048 workgroups (r02): flat within 0.3 % from 384 up
    }
    return {bm, bn};
}

static int pick_splits(long tiles, long kiters) {
    // Small grids are latency-bound (one global-load round trip per K tile, nothing to overlap it with), so
    // split K until there are kSplitTarget workgroups per CU, keeping >= kSplitMinK K-iterations per split.
    const int target = kSplitTarget, mink = kSplitMinK;   // swept in rounds 2-5 (profiles/r0N_sweeps.txt): constants since round 6
    const int forced = (int)cg::opt(cg::OPT_NN_SPLITS);
    if (forced > 0) return (int)std::min<long>(forced, std::max<long>(1, kiters / 2));
    const long want = target < 16 ? (long)target * cg::kNumCU : (long)target;
    int s = 1;
    while (tiles * s < want && kiters / (s * 2) >= mink && s < 64) s *= 2;
    return s;
}

// position-major rows + skipped padding taps (Geom::pmn): the 64-row LDS-direct tiles at K step 32 only
template <int BM, int BN, int WM, int WN>
static void launch_nn_pm(const NNArgs& a, dim3 grid, hipStream_t st) {
    if constexpr (BM == 64 && (BN == 128 || BN == 64)) hipLaunchKernelGGL((igemm_nng_kernel<BM, BN, WM, WN, 32, true>), grid, dim3(256), 0, st, a);
}

template <int BM, int BN, int WM, int WN>
static void launch_nn(const NNArgs& a, dim3 grid, hipStream_t st, bool fast, bool vecb, bool bk32) {
    if (a.g.pmn) { launch_nn_pm<BM, BN, WM, WN>(a, grid, st); return; }
    if (fast && vecb) {
        // LDS-direct loads (igemm_nng_kernel).  CG_NN_GLDS = 1: the 64-row tiles at K step 32 (a pixel's 128 consecutive
        // bytes per 8 lanes; measured inside the replayed step 2.43 -> 1.91 ms for the 64x128 tile), 2: K step 32 for every
        // tile whose Cin allows it, 3: K step 16 as well (64-byte runs per pixel: slower than the register path in the step)
        const long glds = cg::opt(cg::OPT_NN_GLDS);
        if (glds && bk32 && (BM == 64 || glds >= 2)) {
            hipLaunchKernelGGL((igemm_nng_kernel<BM, BN, WM, WN, 32>), grid, dim3(256), 0, st, a);
            return;
        }
        if (glds >= 3) {
            hipLaunchKernelGGL((igemm_nng_kernel<BM, BN, WM, WN, 16>), grid, dim3(256), 0, st, a);
            return;
        }
        // 64-row tiles do only 8-16 MFMAs per wave per K step of 16: give them 32 so the per-tile work
        // (address VALU, LDS stores, barrier) is amortised like in the 128x128 tile
        if (BM == 64 && bk32) hipLaunchKernelGGL((igemm_nn_kernel<BM, BN, WM, WN, true, true, (BM == 64 ? 32 : 16)>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((igemm_nn_kernel<BM, BN, WM, WN, true, true, 16>), grid, dim3(256), 0, st, a);
    }
    else if (fast) hipLaunchKernelGGL((igemm_nn_kernel<BM, BN, WM, WN, true, false, 16>), grid, dim3(256), 0, st, a);
    else if (vecb) hipLaunchKernelGGL((igemm_nn_kernel<BM, BN, WM, WN, false, true, 16>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_nn_kernel<BM, BN, WM, WN, false, false, 16>), grid, dim3(256), 0, st, a);
}

template <int BM, int BN, int WM, int WN>
static void launch_tn(const TNArgs& a, dim3 grid, hipStream_t st, bool veca, bool vecb) {
    if (veca && vecb) hipLaunchKernelGGL((igemm_tn_kernel<BM, BN, WM, WN, true, true>), grid, dim3(256), 0, st, a);
    else if (veca) hipLaunchKernelGGL((igemm_tn_kernel<BM, BN, WM, WN, true, false>), grid, dim3(256), 0, st, a);
    else if (vecb) hipLaunchKernelGGL((igemm_tn_kernel<BM, BN, WM, WN, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_tn_kernel<BM, BN, WM, WN, false, false>), grid, dim3(256), 0, st, a);
}

// LDS-direct weight-gradient kernel (igemm_tng_kernel, K step 16): lean addressing only - whole K tiles of a flat or a lean geometry
static bool tng_flat(const Geom& g) { return g.ntaps == 1 && g.td.r0y0 == 0 && g.td.r0x0 == 0 && tn_lin_out(g); }
static bool tng_ok(const Geom& g, int pchunk, bool veca, bool vecb) {
    if (!cg::opt(cg::OPT_TN_GLDS) || !veca || !vecb || g.M % BK || pchunk % BK) return false;
    return (tn_lin_src(g) && tng_flat(g)) || tn_lean_geom(g);
}

// Position-major K tiles (igemm_tng_kernel mode 2): the share of the layer's MACs that multiply zero padding in per cent, -1 = not this
// geometry (a plain stride-1 convolution with a tap at offset (0, 0) that is valid at every position, whole K tiles of images).
static int tn_pm_share(const Geom& g) {
    if (g.nphase != 1 || g.so != 1 || g.td.ss != 1 || g.td.ngroups != 1 || g.td.sgn != 1 || g.ntaps < 2) return -1;
    if (g.Hout != g.Hg || g.Wout != g.Wg || g.Hg > g.Hv || g.Wg > g.Wv || g.Cin % 4 || g.Cout % 4) return -1;
    const int hw = g.Hg * g.Wg, N = g.M / hw, kh = g.td.kk / g.td.kw;
    if ((long)N * hw != g.M || N % BK) return -1;
    if (g.td.r0y0 > 0 || g.td.r0x0 > 0 || -g.td.r0y0 >= kh || -g.td.r0x0 >= g.td.kw) return -1;
    if ((long)N * g.Hs * g.Ws * g.Cin * 4L >= 0x7fffffffL || (long)g.M * g.Cout * 4L >= 0x7fffffffL) return -1;
    long valid = 0;
    for (int t = 0; t < g.ntaps; ++t) {
        int ty, tx, off;
        tap_decode(g, t, 0, 0, ty, tx, off);
        const int rh = std::min(g.Hg, g.Hv - ty) - std::max(0, -ty), rw = std::min(g.Wg, g.Wv - tx) - std::max(0, -tx);
        if (rh <= 0 || rw <= 0) return -1;
        valid += (long)rh * rw;
    }
    return (int)(100 - 100 * valid / ((long)g.ntaps * hw));
}
// ... used when the padding is at least HALF of CG_PAD_SKIP's share (default 20 -> 10 %: D32_st3's 7x7 at 8x8 38 %, 3x3 at 8x8 16 %, 5x5 at
// 16x16 14 %), or when the image-major tiles cannot run at all (fewer than 16 pixels per image: the View -> Linear head's 1 x 1 grid)
static bool tn_pm_use(const Geom& g, bool image_major_ok) {
    const long thr = cg::opt(cg::OPT_PAD_SKIP);
    if (thr <= 0 || !cg::opt(cg::OPT_TN_GLDS)) return false;
    const int sh = tn_pm_share(g);
    return sh >= 0 && (2 * sh >= thr || !image_major_ok);
}

template <int BM, int BN, int WM, int WN>
static void launch_tng(const TNArgs& a, dim3 grid, hipStream_t st) {
    // (round 5: capping the workgroups per CU with unused dynamic LDS - 3, 2, 1 instead of 4 - to leave slots for the other queues'
    // memory-bound kernels measured 6.05 / 5.95 / 6.10 ms per step against 5.93: profiles/r05_sweeps.txt)
    hipLaunchKernelGGL((igemm_tng_kernel<BM, BN, WM, WN>), grid, dim3(256), 0, st, a, a.pm_n ? 2 : (tng_flat(a.g) ? 1 : 0));
}

static int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

static int finish_geom(Geom& g, long N) {
    const long M = N * g.Hg * g.Wg;
    if (g.Hg <= 0 || g.Wg <= 0) return cg::fail("conv2d: empty output %dx%d", g.Hg, g.Wg);
    if (M > 0x7fffffffL || N * (long)g.Hs * g.Ws * g.Cin > 0x1fffffffL || N * (long)g.Hout * g.Wout * g.Cout > 0x1fffffffL)
        return cg::fail("conv2d: tensor too large for 32-bit element offsets");
    g.M = (int)M;
    const int lw = ilog2_exact(g.Wg), lh = ilog2_exact(g.Hg);
    g.lgW = (lw >= 0 && lh >= 0) ? lw : -1;
    g.lgHW = (lw >= 0 && lh >= 0) ? lw + lh : -1;
    g.Ktot = g.ntaps * g.Cin;
    if (g.ntaps > 64) return cg::fail("conv2d: more than 64 taps");
    int mo[4] = {0, 0, 0, 0};
    for (int ph = 0; ph < g.nphase; ++ph)
        for (int t = 0; t < g.ntaps; ++t) {
            int ty, tx, off;
            tap_decode(g, t, ph >> 1, ph & 1, ty, tx, off);
            mo[ph] = std::min(mo[ph], off);
        }
    g.minoff0 = mo[0]; g.minoff1 = mo[1]; g.minoff2 = mo[2]; g.minoff3 = mo[3];
    return 0;
}

static int check_dims(int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups) {
    if (N <= 0 || Hp <= 0 || Wp <= 0 || Cin <= 0 || Cout <= 0 || kH <= 0 || kW <= 0 || padH < 0 || padW < 0 ||
        (ups != 0 && ups != 1))
        return cg::fail("conv2d: bad geometry N=%d H=%d W=%d Cin=%d Cout=%d k=%dx%d pad=%d,%d ups=%d", N, Hp, Wp, Cin,
                        Cout, kH, kW, padH, padW, ups);
    if (ups && (kH != kW || (kH & 1) == 0 || padH != (kH - 1) / 2 || padW != padH))
        return cg::fail("conv2d: folded upsampling needs an odd square kernel with pad=(k-1)/2 (got %dx%d pad %d,%d)", kH,
                        kW, padH, padW);
    return 0;
}

// plain stride-1 convolution: grid = output pixels, source = the input tensor
static int geom_plain(Geom& g, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW) {
    memset(&g, 0, sizeof(g));
    g.Hg = Hp + 2 * padH - kH + 1; g.Wg = Wp + 2 * padW - kW + 1;
    g.Hv = Hp; g.Wv = Wp; g.Hs = Hp; g.Ws = Wp;
    g.Cin = Cin; g.Cout = Cout;
    g.so = 1; g.Hout = g.Hg; g.Wout = g.Wg;
    g.nphase = 1; g.ntaps = kH * kW;
    g.td.kw = kW; g.td.kk = kH * kW; g.td.ngroups = 1; g.td.sgn = 1; g.td.ss = 1;
    g.td.r0y0 = g.td.r0y1 = -padH; g.td.r0x0 = g.td.r0x1 = -padW;
    return finish_geom(g, N);
}

// upsample(2) -> conv, forward / weight-gradient view: 4 phases over the low-res grid
static int geom_phase_fwd(Geom& g, int N, int Hp, int Wp, int Cin, int Cout, int k, int pad) {
    memset(&g, 0, sizeof(g));
    const int kp = phase_kp(k, pad);
    g.Hg = Hp; g.Wg = Wp; g.Hv = Hp; g.Wv = Wp; g.Hs = Hp; g.Ws = Wp;
    g.Cin = Cin; g.Cout = Cout;
    g.so = 2; g.Hout = 2 * Hp; g.Wout = 2 * Wp;
    g.nphase = 4; g.ntaps = kp * kp;
    g.td.kw = kp; g.td.kk = kp * kp; g.td.ngroups = 1; g.td.sgn = 1; g.td.ss = 1;
    g.td.r0y0 = g.td.r0x0 = (0 - pad) >> 1;
    g.td.r0y1 = g.td.r0x1 = (1 - pad) >> 1;
    return finish_geom(g, N);
}

// data gradient w.r.t. the low-res input: one GEMM whose taps run over (phase, ry', rx') of dy [N,2Hp,2Wp,CoutF]
static int geom_phase_dgrad(Geom& g, int N, int Hp, int Wp, int CinF, int CoutF, int k, int pad) {
    memset(&g, 0, sizeof(g));
    const int kp = phase_kp(k, pad);
    g.Hg = Hp; g.Wg = Wp; g.Hv = Hp; g.Wv = Wp; g.Hs = 2 * Hp; g.Ws = 2 * Wp;
    g.Cin = CoutF; g.Cout = CinF;
    g.so = 1; g.Hout = Hp; g.Wout = Wp;
    g.nphase = 1; g.ntaps = 4 * kp * kp;
    g.td.kw = kp; g.td.kk = kp * kp; g.td.ngroups = 4; g.td.sgn = -1; g.td.ss = 2;
    g.td.r0y0 = g.td.r0x0 = (0 - pad) >> 1;
    g.td.r0y1 = g.td.r0x1 = (1 - pad) >> 1;
    return finish_geom(g, N);
}

struct NNPlan { TileCfg tc; int splits; int kchunk; bool pm; };
static long pad_skip_valid(const Geom& g, const TileCfg& tc);
static NNPlan plan_nn(const Geom& g, int ngroups, bool allow_pm = true) {
    NNPlan p;
    const int zdim = g.nphase * ngroups;
    p.tc = pick_tile(g.M, g.Cout, zdim);
    p.pm = false;
    const long valid = (allow_pm && ngroups == 1 && g.Cin % 32 == 0) ? pad_skip_valid(g, p.tc) : 0;
    if (valid > 0) {
        // position-major tiles (Geom::pmn): K units of equal length cut out of every tile's VALID taps; gridDim.y = the units of an interior
        // tile.  Round 5 aimed at one unit per CU (61 K tiles for D's 7x7 layer at batch 128: 312 workgroups, 1.2 per CU, the short last
        // units of every tile in the way); round 6 measured the unit length itself: 28 K tiles (592 workgroups) run the layer in 96 us
        // alone against 122 (61), 109 (49 / 33 / 25 / 20), 123 (40), and the step at 5.635 / 11.27 / 8.33 ms (configs 2 / 5 / 3) against
        // 5.678 / 11.36 / 8.42; 20 and 33 sit between (profiles/r06_sweeps.txt)
        constexpr long kPmUnit = 28;
        long unit = kPmUnit;
        const int forced = (int)cg::opt(cg::OPT_NN_SPLITS);
        if (forced > 0) unit = cg::cdiv(g.Ktot / 32, forced);
        p.kchunk = (int)std::min<long>(unit * 32, g.Ktot);
        p.splits = cg::cdiv(g.Ktot, p.kchunk);
        p.pm = true;
        return p;
    }
    const long tiles = (long)cg::cdiv(g.M, p.tc.bm) * cg::cdiv(g.Cout, p.tc.bn) * zdim;
    const long kiters = cg::cdiv(g.Ktot, BK);
    p.splits = pick_splits(tiles, kiters);
    p.kchunk = cg::cdiv(cg::cdiv(kiters, p.splits) * BK, 32) * 32;
    p.splits = cg::cdiv(g.Ktot, p.kchunk);
    return p;
}
static size_t nn_ws_bytes(const Geom& g, const NNPlan& p, int ngroups) {
    size_t b = p.splits > 1 ? (size_t)p.splits * ngroups * g.nphase * g.M * g.Cout * sizeof(float) : 0;
    if (p.pm) b = std::max(b, nn_ws_bytes(g, plan_nn(g, ngroups, false), ngroups));   // run_nn may fall back (unaligned operands, statistics)
    return b;
}

struct TNPlan { TileCfg tc; int splits; int pchunk; bool pm; };
static TNPlan plan_tn(const Geom& g, int ngroups, bool allow_pm = true) {
    TNPlan p;
    int bn = g.Cout > 64 ? 128 : (g.Cout > 32 ? 64 : 32);
    int bm = g.Ktot > 64 ? 128 : 64;
    if (bn == 32) bm = 128;
    p.tc = {bm, bn};
    tile_forced(cg::OPT_TN_TILE, p.tc);
    bm = p.tc.bm; bn = p.tc.bn;
    const long tiles = (long)cg::cdiv(g.Ktot, bm) * cg::cdiv(g.Cout, bn) * g.nphase * ngroups;
    const long piters = cg::cdiv(g.M, BK);
    const int smax = kTnSplitMax, tgt = kTnTarget;
    const int forced = (int)cg::opt(cg::OPT_TN_SPLITS);
    p.pm = allow_pm && tn_pm_use(g, tng_ok(g, BK, true, true));
    if (p.pm) {
        // position-major tiles: a split is a share of every workgroup's OWN tile list, so any count works - the one that fills tgt
        // workgroups per CU most exactly (D32_st3's 5x5 layer: 13 tiles x 59 = 767 workgroups 119 us, x 64 = 832 130 us), with >= 8 K
        // tiles per workgroup on average (profiles/r06_sweeps.txt)
        const long kt = std::max<long>(1, piters * (100 - tn_pm_share(g)) / 100);
        long sp = forced > 0 ? forced : std::min<long>((long)tgt * cg::kNumCU / std::max<long>(1, tiles), kt / 8);
        p.splits = (int)std::max<long>(1, std::min<long>(sp, smax));
        p.pchunk = 0;
        return p;
    }
    int s = 1;
    if (forced > 0) s = (int)std::min<long>(forced, std::max<long>(1, piters));
    else
    while (tiles * s < (long)tgt * cg::kNumCU && piters / (s * 2) >= 8 && s < smax) s *= 2;
    p.pchunk = cg::cdiv(piters, s) * BK;
    p.splits = cg::cdiv(g.M, p.pchunk);
    return p;
}
static size_t tn_ws_bytes(const Geom& g, const TNPlan& p, int ngroups) {
    // a position-major plan falls back to the image-major one for unaligned operands: room for either
    const int splits = p.pm ? std::max(p.splits, plan_tn(g, ngroups, false).splits) : p.splits;
    return (size_t)splits * ngroups * g.nphase * ((size_t)g.Ktot + 1) * g.Cout * sizeof(float);
}

struct Epi { int act; float slope; const float* const* alpha; float* const* y_act; float* stats; };

// Position-major rows with the zero-padding taps skipped (Geom::pmn): a plain stride-1 convolution whose padding is a real share of
// its MACs (CG_PAD_SKIP = the least share in per cent, 0 = off), batch a power of two and a multiple of the 64-row tile.  Returns the
// number of (pixel position, tap) pairs inside the image, 0 = not this launch.
static long pad_skip_valid(const Geom& g, const TileCfg& tc) {
    const long thr = cg::opt(cg::OPT_PAD_SKIP);
    if (thr <= 0 || !cg::opt(cg::OPT_NN_GLDS) || !cg::opt(cg::OPT_GEMM_BK32)) return 0;
    if (g.nphase != 1 || g.so != 1 || g.td.ngroups != 1 || g.td.ss != 1 || g.ntaps < 9 || tc.bm != 64 || !(tc.bn == 128 || tc.bn == 64)) return 0;
    const int hw = g.Hg * g.Wg, N = g.M / hw;
    if (N * hw != g.M || N % 64 || ilog2_exact(N) < 0 || g.Cout % tc.bn || (long)g.M * g.Cout * 4L >= 0x7fffffffL) return 0;
    long valid = 0;
    for (int oy = 0; oy < g.Hg; ++oy)
        for (int ox = 0; ox < g.Wg; ++ox)
            for (int t = 0; t < g.ntaps; ++t) {
                int ty, tx, off;
                tap_decode(g, t, 0, 0, ty, tx, off);
                valid += (unsigned)(oy + ty) < (unsigned)g.Hv && (unsigned)(ox + tx) < (unsigned)g.Wv;
            }
    return (long)hw * g.ntaps * (100 - thr) >= valid * 100 ? valid : 0;
}

static int run_nn(hipStream_t st, const Geom& g, int ngroups, const float* const* x, const float* const* w,
                  const float* const* bias, float* const* y, void* ws, size_t ws_bytes, const char* who,
                  const Epi* ep = nullptr) {
    CG_REQUIRE(ngroups >= 1 && ngroups <= MAXG, "%s: 1..%d groups per launch", who, MAXG);
    NNPlan p = plan_nn(g, ngroups);
    {
        bool al16 = true;
        for (int i = 0; i < ngroups; ++i) al16 = al16 && x[i] && w[i] && (uintptr_t)x[i] % 16 == 0 && (uintptr_t)w[i] % 16 == 0;
        if (p.pm && (!al16 || g.Cout % 4 || (ep && ep->stats))) p = plan_nn(g, ngroups, false);   // the LDS-direct kernel cannot: image-major plan
    }
    const size_t need = nn_ws_bytes(g, p, ngroups);
    CG_REQUIRE(need == 0 || (ws && ws_bytes >= need), "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    NNArgs a;
    memset(&a, 0, sizeof(a));
    bool al = true, alw = true;
    for (int i = 0; i < ngroups; ++i) {
        CG_REQUIRE(x[i] && w[i] && y[i], "%s: null pointer (group %d)", who, i);
        al = al && ((uintptr_t)x[i] % 16 == 0);
        alw = alw && ((uintptr_t)w[i] % 16 == 0);
    }
    set4(a.x0, a.x1, a.x2, a.x3, x, ngroups);
    set4(a.w0, a.w1, a.w2, a.w3, w, ngroups);
    set4(a.b0, a.b1, a.b2, a.b3, bias, ngroups);
    set4(a.y0, a.y1, a.y2, a.y3, y, ngroups);
    a.part = (float*)ws; a.ngroups = ngroups; a.g = g;
    a.kchunk = p.kchunk; a.nsplit = p.splits;
    a.xcd_swizzle = (int)cg::opt(cg::OPT_XCD_SWIZZLE);
    if (ep && ep->act) {
        CG_REQUIRE(ep->act == 1 || ep->act == 2, "%s: unknown activation %d", who, ep->act);
        CG_REQUIRE(ep->y_act, "%s: fused activation needs y_act", who);
        for (int i = 0; i < ngroups; ++i) {
            CG_REQUIRE(ep->y_act[i], "%s: null y_act (group %d)", who, i);
            CG_REQUIRE(ep->act != 1 || (ep->alpha && ep->alpha[i]), "%s: PReLU epilogue needs the slope pointer (group %d)", who, i);
        }
        a.act = ep->act; a.slope = ep->slope;
        set4(a.al0, a.al1, a.al2, a.al3, ep->act == 1 ? ep->alpha : nullptr, ngroups);
        set4(a.z0, a.z1, a.z2, a.z3, ep->y_act, ngroups);
    }
    if (ep && ep->stats) {
        CG_REQUIRE(ngroups == 1 && p.splits == 1, "%s: epilogue statistics need a single-group, unsplit launch", who);
        a.stats = ep->stats;
    }
    const bool fast = (g.Cin % BK == 0) && al;
    const bool vecb = (g.Cout % 4 == 0) && alw;
    const bool bk32 = cg::opt(cg::OPT_GEMM_BK32) != 0 && (g.Cin % 32 == 0) && (p.kchunk % 32 == 0);
    if (a.xcd_swizzle & 4) {
        // weights-stationary XCDs only where they move fewer bytes: an r x c XCD grid over (row tiles) x (column tiles) fetches
        // c |x| + r |w| per phase - row ranges (r = 8, c = 1) against (8 / ntn, ntn).  conv1's forward: |x| = |w| = 4.2 MB -> stationary
        // (161 -> 68 MB measured); conv2's direct data gradient: |x| = 33.5, |w| = 8.4 MB -> row ranges (118 MB; 258 MB stationary)
        const int ntn = cg::cdiv(g.Cout, p.tc.bn);
        const double xb = (double)(g.M / (g.Hg * g.Wg)) * g.Hs * g.Ws * g.Cin * 4.0, wb = (double)g.Ktot * g.Cout * 4.0;
        if (!(ntn == 2 || ntn == 4 || ntn == 8) || ntn * xb + (8 / ntn) * wb >= xb + 8 * wb) a.xcd_swizzle &= ~4;
    }
    if (p.pm) {
        a.g.pmn = g.M / (g.Hg * g.Wg);
        a.g.pm_lg = ilog2_exact(a.g.pmn);
    }
    dim3 grid(cg::cdiv(g.M, p.tc.bm) * cg::cdiv(g.Cout, p.tc.bn), p.splits, g.nphase * ngroups);
    with_block_tile(p.tc, [&](auto t) {
        using T = decltype(t);
        launch_nn<T::BM, T::BN, T::WM, T::WN>(a, grid, st, fast, vecb, bk32);
    });
    CG_LAUNCH_CHECK();
    if (p.splits > 1) {
        const long PMN = (long)ngroups * g.nphase * g.M * g.Cout;
        bool v4 = g.Cout % 4 == 0 && (uintptr_t)ws % 16 == 0;
        for (int i = 0; i < ngroups; ++i)
            v4 = v4 && (uintptr_t)y[i] % 16 == 0 && (!bias || (uintptr_t)bias[i] % 16 == 0) && (!a.act || (uintptr_t)ep->y_act[i] % 16 == 0);
        if ((PMN >= 256L * 1024 || p.splits < 8) && v4)
            hipLaunchKernelGGL((nn_splitk_reduce_kernel<1, true>), dim3(cg::ew_grid(PMN / 4)), dim3(256), 0, st, a, p.splits);
        else if (PMN >= 256L * 1024 || p.splits < 8)
            hipLaunchKernelGGL(nn_splitk_reduce_kernel<1>, dim3(cg::ew_grid(PMN)), dim3(256), 0, st, a, p.splits);
        else
            hipLaunchKernelGGL(nn_splitk_reduce_kernel<8>, dim3((unsigned)cg::cdiv(PMN, 32)), dim3(256), 0, st, a, p.splits);
        CG_LAUNCH_CHECK();
    }
    return 0;
}

static int conv_geom(Geom& g, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups) {
    if (check_dims(N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 1;
    return ups ? geom_phase_fwd(g, N, Hp, Wp, Cin, Cout, kH, padH) : geom_plain(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW);
}

}  // namespace

#ifdef CG_TRACE
extern "C" int cg_debug_set_trace(void* p) {
    unsigned long long* q = (unsigned long long*)p;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &q, sizeof(q)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" {

size_t cg_conv2d_workspace_bytes_grouped(int ngroups, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH,
                                         int padW, int ups) {
    Geom g;
    if (ngroups < 1 || ngroups > MAXG || conv_geom(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 0;
    return nn_ws_bytes(g, plan_nn(g, ngroups), ngroups);
}
size_t cg_conv2d_workspace_bytes(int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups) {
    return cg_conv2d_workspace_bytes_grouped(1, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups);
}

// rows of the statistics buffer an epilogue-statistics launch writes (0: this geometry runs split-K or skinny, take the
// statistics with cg_bn_stats instead)
size_t cg_conv2d_stats_rows(int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups) {
    Geom g;
    if (conv_geom(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 0;
    if (cg::skinny_ok(1, Cin, Cout, kH, kW, padH, padW, ups)) return 0;
    const NNPlan p = plan_nn(g, 1, false);   // run_nn launches the image-major plan whenever statistics are asked for: query THAT plan
    if (p.splits != 1) return 0;
    const int wm = p.tc.bn == 32 ? 4 : 2;
    return (size_t)g.nphase * cg::cdiv(g.M, p.tc.bm) * wm;
}

int cg_conv2d_forward_ex(void* stream, int ngroups, const float* const* x, const float* const* wpk, const float* const* bias,
                         float* const* y, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW,
                         int ups, int act, float slope, const float* const* alpha, float* const* y_act, float* stats,
                         void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && wpk && y, "cg_conv2d_forward_ex: null pointer");
    Geom g;
    if (conv_geom(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 1;
    CG_REQUIRE(!cg::skinny_ok(ngroups, Cin, Cout, kH, kW, padH, padW, ups) || (act == 0 && !stats),
               "cg_conv2d_forward_ex: no fused epilogue on the skinny (<= 4 output planes) path");
    if (act == 0 && !stats)
        return cg_conv2d_forward_grouped(stream, ngroups, x, wpk, bias, y, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, ws,
                                         ws_bytes);
    Epi ep{act, slope, alpha, y_act, stats};
    return run_nn(cg::S(stream), g, ngroups, x, wpk, bias, y, ws, ws_bytes, "cg_conv2d_forward_ex", &ep);
}

int cg_conv2d_forward_grouped(void* stream, int ngroups, const float* const* x, const float* const* wpk,
                              const float* const* bias, float* const* y, int N, int Hp, int Wp, int Cin, int Cout, int kH,
                              int kW, int padH, int padW, int ups, void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && wpk && y, "cg_conv2d_forward_grouped: null pointer");
    Geom g;
    if (conv_geom(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 1;
    if (cg::skinny_ok(ngroups, Cin, Cout, kH, kW, padH, padW, ups) && x[0] && wpk[0] && y[0] && (uintptr_t)x[0] % 16 == 0 &&
        (long)N * Hp * Wp < 0x7fffffffL) {
        const float* b0 = bias ? bias[0] : nullptr;
        if (cg::opt(cg::OPT_SKINNY) == 1 && cg::skinny_mfma_ok(Cin, Cout, Hp, Wp)) {
            if (cg::skinny_mfma_forward(cg::S(stream), x[0], wpk[0], b0, y[0], N, Hp, Wp, Cin, Cout)) return 1;
        }
        else cg::skinny_valu_forward(cg::S(stream), x[0], wpk[0], b0, y[0], N, Hp, Wp, Cin, Cout);
        CG_LAUNCH_CHECK();
        return 0;
    }
    if (cg::wino3_geom_ok(ngroups, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) {   // fused F(2x2,3x3): csrc/wino3.hip
        const int rc = cg::wino3_forward(cg::S(stream), ngroups, x, wpk, bias, y, N, Hp, Wp);
        if (rc) return rc < 0 ? 1 : 0;
    }
    return run_nn(cg::S(stream), g, ngroups, x, wpk, bias, y, ws, ws_bytes, "cg_conv2d_forward_grouped");
}

int cg_conv2d_forward(void* stream, const float* x, const float* wpk, const float* bias, float* y, int N, int Hp, int Wp,
                      int Cin, int Cout, int kH, int kW, int padH, int padW, int ups, void* ws, size_t ws_bytes) {
    return cg_conv2d_forward_grouped(stream, 1, &x, &wpk, bias ? &bias : nullptr, &y, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW,
                                     ups, ws, ws_bytes);
}

size_t cg_conv2d_dgrad_ups2_workspace_bytes(int N, int Hp, int Wp, int Cin, int Cout, int k, int pad) {
    Geom g;
    if (check_dims(N, Hp, Wp, Cin, Cout, k, k, pad, pad, 1)) return 0;
    if (geom_phase_dgrad(g, N, Hp, Wp, Cin, Cout, k, pad)) return 0;
    return nn_ws_bytes(g, plan_nn(g, 1), 1);
}

int cg_conv2d_dgrad_ups2(void* stream, const float* dy, const float* wb_ph, float* dx_lo, int N, int Hp, int Wp, int Cin,
                         int Cout, int k, int pad, void* ws, size_t ws_bytes) {
    CG_REQUIRE(dy && wb_ph && dx_lo, "cg_conv2d_dgrad_ups2: null pointer");
    Geom g;
    if (check_dims(N, Hp, Wp, Cin, Cout, k, k, pad, pad, 1)) return 1;
    if (geom_phase_dgrad(g, N, Hp, Wp, Cin, Cout, k, pad)) return 1;
    return run_nn(cg::S(stream), g, 1, &dy, &wb_ph, nullptr, &dx_lo, ws, ws_bytes, "cg_conv2d_dgrad_ups2");
}

static size_t wgrad_ws_bytes_groups(int ngroups, int maxg, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups) {
    Geom g;
    if (ngroups < 1 || ngroups > maxg || conv_geom(g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 0;
    const size_t reg = tn_ws_bytes(g, plan_tn(g, ngroups), ngroups);
    return cg::skinny_ok(ngroups, Cin, Cout, kH, kW, padH, padW, ups) ? std::max(reg, cg::skinny_wgrad_ws_bytes(Cin, Cout)) : reg;
}
// The size query doubles as the capability check of the entry point it belongs to (0 = this launch does not exist): <= MAXG groups of
// separate tensors for cg_conv2d_wgrad_grouped / _deferred, <= kMaxStridedGroups equally spaced ones for cg_conv2d_wgrad_strided.
size_t cg_conv2d_wgrad_workspace_bytes_grouped(int ngroups, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW,
                                               int padH, int padW, int ups) {
    return wgrad_ws_bytes_groups(ngroups, MAXG, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups);
}
size_t cg_conv2d_wgrad_workspace_bytes_strided(int ngroups, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW,
                                               int padH, int padW, int ups) {
    return wgrad_ws_bytes_groups(ngroups, kMaxStridedGroups, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups);
}
size_t cg_conv2d_wgrad_workspace_bytes(int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW,
                                       int ups) {
    return cg_conv2d_wgrad_workspace_bytes_grouped(1, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups);
}

namespace {
int wgrad_impl(void* stream, int ngroups, const float* const* x, const float* const* dy, float* const* gw, float* const* gb, int N,
               int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups, float scale, void* ws, size_t ws_bytes,
               bool defer, long xgs = 0, long dgs = 0, long gws = 0, bool gemm_only = false);
}  // namespace

int cg_conv2d_wgrad_grouped(void* stream, int ngroups, const float* const* x, const float* const* dy, float* const* gw,
                            float* const* gb, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW,
                            int ups, float scale, void* ws, size_t ws_bytes) {
    return wgrad_impl(stream, ngroups, x, dy, gw, gb, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, scale, ws, ws_bytes, false);
}

int cg_conv2d_wgrad_grouped_deferred(void* stream, int ngroups, const float* const* x, const float* const* dy, float* const* gw,
                                     float* const* gb, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW,
                                     int ups, float scale, void* ws, size_t ws_bytes) {
    return wgrad_impl(stream, ngroups, x, dy, gw, gb, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, scale, ws, ws_bytes, true);
}

// ngroups (<= 16) weight gradients of ONE geometry whose tensors are equally spaced in memory - group g reads x + g*x_stride and
// dy + g*dy_stride (floats) and accumulates into gw + g*gw_stride - in one GEMM launch and one reduction.  What the Winograd-domain
// weight gradient of winograd.hip is: 16 independent [tiles x Cin]^T [tiles x 4 Cout] products, one per transform position
// (four launches of four groups through cg_conv2d_wgrad_grouped before round 4).  No bias gradients.  Workspace:
// cg_conv2d_wgrad_workspace_bytes_strided(ngroups, ...).
int cg_conv2d_wgrad_strided(void* stream, int ngroups, const float* x, long x_stride, const float* dy, long dy_stride, float* gw,
                            long gw_stride, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups,
                            float scale, void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && dy && gw && x_stride > 0 && dy_stride > 0 && gw_stride > 0, "cg_conv2d_wgrad_strided: bad arguments");
    CG_REQUIRE(ngroups >= 1 && ngroups <= kMaxStridedGroups, "cg_conv2d_wgrad_strided: 1..%d groups per launch", kMaxStridedGroups);
    return wgrad_impl(stream, ngroups, &x, &dy, &gw, nullptr, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, scale, ws, ws_bytes, false,
                      x_stride, dy_stride, gw_stride);
}

// The weight-gradient GEMM alone: the split partial sums [splits][phases][taps*Cin][Cout] are left in ws, nothing is reduced into a
// gradient (exported so that the kernel can be timed / profiled in isolation - bench.py's roofline entry; not part of a training step).
int cg_conv2d_wgrad_gemm(void* stream, const float* x, const float* dy, int N, int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH,
                         int padW, int ups, void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && dy && ws, "cg_conv2d_wgrad_gemm: null pointer");
    CG_REQUIRE(!cg::skinny_ok(1, Cin, Cout, kH, kW, padH, padW, ups), "cg_conv2d_wgrad_gemm: this geometry runs the skinny kernel, not the GEMM");
    float* gw = (float*)ws;   // never written: the reduction is skipped
    return wgrad_impl(stream, 1, &x, &dy, &gw, nullptr, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, 1.f, ws, ws_bytes, false, 0, 0, 0, true);
}

namespace {
// the two staging families of the weight gradient (tng: LDS-direct loads)
void launch_tn_tile(const TNArgs& a, const TileCfg& tc, bool tng, dim3 grid, hipStream_t st, bool veca, bool vecb) {
    with_block_tile(tc, [&](auto t) {
        using T = decltype(t);
        if (tng) launch_tng<T::BM, T::BN, T::WM, T::WN>(a, grid, st);
        else launch_tn<T::BM, T::BN, T::WM, T::WN>(a, grid, st, veca, vecb);
    });
}

int wgrad_impl(void* stream, int ngroups, const float* const* x, const float* const* dy, float* const* gw, float* const* gb, int N,
               int Hp, int Wp, int Cin, int Cout, int kH, int kW, int padH, int padW, int ups, float scale, void* ws, size_t ws_bytes,
               bool defer, long xgs, long dgs, long gws_, bool gemm_only) {
    CG_REQUIRE(x && dy && gw, "cg_conv2d_wgrad: null pointer");
    const bool strided = xgs != 0;     // equally spaced groups: only x[0] / dy[0] / gw[0] are pointers
    CG_REQUIRE(ngroups >= 1 && ngroups <= (strided ? kMaxStridedGroups : MAXG), "cg_conv2d_wgrad: 1..%d groups per launch", strided ? kMaxStridedGroups : MAXG);
    CG_REQUIRE(!strided || (!gb && !defer), "cg_conv2d_wgrad: strided groups carry no bias gradient and are not deferred");
    TNArgs a;
    memset(&a, 0, sizeof(a));
    if (conv_geom(a.g, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups)) return 1;
    const Geom& g = a.g;
    // 1. the shortcuts: a skinny layer's own kernels (their partial planes finish like the GEMM's), the head's one-kernel gradient
    if (!strided && cg::skinny_ok(ngroups, Cin, Cout, kH, kW, padH, padW, ups) && x[0] && dy[0] && gw[0] && (uintptr_t)x[0] % 16 == 0 && ws &&
        ws_bytes >= cg::skinny_wgrad_ws_bytes(Cin, Cout) && (long)N * Hp * Wp < 0x7fffffffL) {
        hipStream_t st = cg::S(stream);
        const long npix = (long)N * Hp * Wp;
        const long ppb = (npix + cg::kSkinnyWgradBlocks - 1) / cg::kSkinnyWgradBlocks;
        int blocks = (int)((npix + ppb - 1) / ppb);
        float* part = (float*)ws;
        float* bpart = part + (size_t)cg::kSkinnyWgradBlocks * 9 * Cin * Cout;
        float* gb0 = gb ? gb[0] : nullptr;
        if (cg::opt(cg::OPT_SKINNY) == 1 && cg::skinny_mfma_ok(Cin, Cout, Hp, Wp)) {
            // 256 partial planes: the kernel itself measures the same with 512 (18.0 / 18.8 us at batch 128), the reduction behind it 18 -> 12.6 us
            blocks = cg::skinny_mfma_wgrad(st, x[0], dy[0], part, gb0 ? bpart : nullptr, N, Hp, Wp, Cin, Cout, cg::kSkinnyWgradBlocks / 2);
            if (blocks < 0) return 1;
        }
        else cg::skinny_valu_wgrad(st, x[0], dy[0], part, gb0 ? bpart : nullptr, N, Hp, Wp, Cin, Cout, blocks, ppb);
        CG_LAUNCH_CHECK();
        const cg::WgradParts parts{part, gb0 ? bpart : nullptr, gw, gb, 0, 1, blocks, Cin, Cout, 3, 3, 1, 0, scale};
        return cg::wgrad_finish(st, parts, defer);
    }
    // nn.View -> nn.Linear (an H x W kernel on the H x W map, 1 x 1 grid): one kernel straight into gradWeight (headwg.hip)
    if (!strided && !gemm_only && ngroups == 1 && !ups && kH == Hp && kW == Wp && padH == 0 && padW == 0 && cg::opt(cg::OPT_PAD_SKIP) > 0 &&
        cg::opt(cg::OPT_TN_GLDS) && cg::head_wgrad_ok(N, kH * kW, Cin, Cout) && x[0] && dy[0] && gw[0] && (uintptr_t)x[0] % 16 == 0 &&
        (uintptr_t)dy[0] % 16 == 0 && (uintptr_t)gw[0] % 4 == 0)
        return cg::head_wgrad(cg::S(stream), x[0], dy[0], gw[0], gb ? gb[0] : nullptr, N, kH * kW, Cin, Cout, scale) != 0;
    // 2. the TN launch: split partials [splits][groups * phases][taps * Cin][Cout] and, behind them, the bias partials into ws
    TNPlan p = plan_tn(g, ngroups);
    const size_t need = tn_ws_bytes(g, p, ngroups);
    CG_REQUIRE(ws && ws_bytes >= need, "cg_conv2d_wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
    const int nptr = strided ? 1 : ngroups;
    bool veca = Cin % 4 == 0, vecb = Cout % 4 == 0, any_gb = false;
    for (int i = 0; i < nptr; ++i) {
        CG_REQUIRE(x[i] && dy[i] && gw[i], "cg_conv2d_wgrad: null pointer (group %d)", i);
        veca = veca && ((uintptr_t)x[i] % 16 == 0);
        vecb = vecb && ((uintptr_t)dy[i] % 16 == 0);
        any_gb = any_gb || (gb && gb[i]);
    }
    if (strided) { veca = veca && xgs % 4 == 0; vecb = vecb && dgs % 4 == 0; }
    if (p.pm && !(veca && vecb)) p = plan_tn(g, ngroups, false);   // unaligned operands: the image-major plan (the workspace holds either)
    a.xgs = xgs; a.dgs = dgs;
    set4(a.x0, a.x1, a.x2, a.x3, x, nptr);
    set4(a.d0, a.d1, a.d2, a.d3, dy, nptr);
    a.ngroups = ngroups; a.part = (float*)ws; a.pchunk = p.pchunk;
    a.xcd_swizzle = (int)cg::opt(cg::OPT_XCD_SWIZZLE);
    const int ZP = ngroups * g.nphase;
    const long wplane = (long)g.Ktot * g.Cout;              // one (group, phase) slab of weight partials
    a.bias_part = any_gb ? (float*)ws + (size_t)p.splits * ZP * wplane : nullptr;
    hipStream_t st = cg::S(stream);
    dim3 grid(cg::cdiv(g.Ktot, p.tc.bm) * cg::cdiv(g.Cout, p.tc.bn), p.splits, ZP);
    if (p.pm && veca && vecb) a.pm_n = g.M / (g.Hg * g.Wg);
    launch_tn_tile(a, p.tc, a.pm_n || tng_ok(g, p.pchunk, veca, vecb), grid, st, veca, vecb);
    CG_LAUNCH_CHECK();
    if (gemm_only) return 0;   // cg_conv2d_wgrad_gemm: the partial sums stay in ws
    // 3. the finish: the partials into the canonical gradients, now or with the stream's other deferred ones
    const cg::WgradParts parts{(const float*)ws, a.bias_part, gw, gb, strided ? gws_ : 0, ngroups, p.splits, Cin, Cout, kH, kW, padH, ups, scale};
    return cg::wgrad_finish(st, parts, defer);
}

}  // namespace

int cg_conv2d_wgrad(void* stream, const float* x, const float* dy, float* gw, float* gb, int N, int Hp, int Wp, int Cin,
                    int Cout, int kH, int kW, int padH, int padW, int ups, float scale, void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && dy && gw, "cg_conv2d_wgrad: null pointer");
    return cg_conv2d_wgrad_grouped(stream, 1, &x, &dy, &gw, &gb, N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups, scale, ws,
                                   ws_bytes);
}

}  // extern "C"
