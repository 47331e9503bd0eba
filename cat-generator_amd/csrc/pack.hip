// The weight re-packing after every parameter update: Torch7's canonical [Cout][Cin][kH][kW] weights -> the operands of gemm.hip,
//   plain:  wf[tap*Cin+ci][Cout] (forward, weight gradient), wb[(KK-1-tap)*Cout+co][Cin] (data gradient)
//   behind nn.SpatialUpSamplingNearest(2): the four phase-summed k' x k' kernels of the same two views (gemm.hip's header)
// CG_PACK_WIDE (common.h) picks the wide launches (the default) or the kernels they replaced; the bytes are the same
// (tests/test_gpu_pack_wide.py).  The Winograd filter packs are in winograd.hip and wino3.hip.
#include "common.h"

namespace {

using cg::phase_kp;
using cg::phase_map;

// canonical [Cout][Cin][KK] -> wf[tap*Cin+ci][Cout], wb[(KK-1-tap)*Cout+co][Cin]
// (the parameters change every step, so this runs every step).  One workgroup owns a 32 ci x 32 co block: thread
// (ci_l, co_l + 8j) reads its canonical tap run, writes wb directly (ci-fastest, coalesced) and transposes the
// 32x32 plane of each tap through LDS for wf (co-fastest).
// wb_map != 0: wb receives the row-permuted canonical matrix wbT[co][tap*Cin + ci] instead of the flipped-tap data-gradient
// operand - the backward operand of a LINEAR layer that consumes an NHWC map directly (its canonical [out][C*H*W] weight is
// the canonical weight of a k = H x W convolution on that map; see cg_pack_conv_weight_map).
__device__ __forceinline__ void pack_block_tap(float (&sh)[32][33], const float* w, float* wf, float* wb, int Cout, int Cin, int KK,
                                               bool wb_map, int ci0, int co0, int tap) {
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + lo, co_l = hi + 8 * j, co = co0 + co_l;
        float v = 0.f;
        if (ci < Cin && co < Cout) {
            v = w[((long)co * Cin + ci) * KK + tap];
            if (wb) wb[wb_map ? ((long)co * KK + tap) * Cin + ci : ((long)(KK - 1 - tap) * Cout + co) * Cin + ci] = v;
        }
        sh[lo][co_l] = v;
    }
    if (wf) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + lo, ci_l = hi + 8 * j, ci = ci0 + ci_l;
            if (ci < Cin && co < Cout) wf[((long)tap * Cin + ci) * Cout + co] = sh[ci_l][lo];
        }
    }
}
// one tap plane per workgroup: KK independent workgroups instead of KK serial rounds
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* w, float* wf, float* wb, int Cout, int Cin, int KK, int wb_map) {
    __shared__ float sh[32][33];
    pack_block_tap(sh, w, wf, wb, Cout, Cin, KK, wb_map != 0, blockIdx.x * 32, blockIdx.y * 32, blockIdx.z);
}

// The same for up to kPackBatch layers in ONE launch (all of D32_st3's 28 convolution / linear layers re-pack after every
// Adam step: 28 launches of a few microseconds each otherwise).  A workgroup finds its layer by its block index.
constexpr int kPackBatch = 48;
struct PackBatch {
    const float* w[kPackBatch]; float* wf[kPackBatch]; float* wb[kPackBatch];
    int Cout[kPackBatch], Cin[kPackBatch], KK[kPackBatch], first[kPackBatch + 1];
    unsigned long long map_mask;   // bit e: layer e wants the wbT layout (see pack_weight_kernel)
    int n;
};
__global__ __launch_bounds__(256) void pack_weight_batch_kernel(PackBatch b) {
    __shared__ float sh[32][33];
    int e = 0;
    while (e + 1 < b.n && (int)blockIdx.x >= b.first[e + 1]) ++e;
    const int Cout = b.Cout[e], Cin = b.Cin[e], KK = b.KK[e];
    const int nbx = (Cin + 31) / 32, nby = (Cout + 31) / 32;
    int r = (int)blockIdx.x - b.first[e];
    const int bx = r % nbx; r /= nbx;
    const int by = r % nby;
    pack_block_tap(sh, b.w[e], b.wf[e], b.wb[e], Cout, Cin, KK, (b.map_mask >> e) & 1ull, bx * 32, by * 32, r / nby);
}

// The wide form of the batch pack (CG_PACK_WIDE, the default).  The kernel above reads w[co][ci][tap] with a lane stride of KK floats
// and once per tap: KK workgroups fetch the same lines for 4 bytes of each 32-byte sector (View -> Linear(20480, 256) as an 8 x 8 kernel:
// 64 times; a linear or 1 x 1 layer has none of this and keeps that body).  Here a workgroup owns a 32 ci x 32 co block and a CHUNK of
// up to kPackTc taps (all of a 3 x 3 kernel, 7 of the 49 of a 7 x 7, 8 of the map's 64): every (co, ci) contributes one contiguous run
// of the chunk's taps, read once into LDS, and wb (ci-fastest) and wf (co-fastest) are both stored in whole 128-byte rows from there
// (row strides 9 and 289 words: no bank conflicts either way).
// The transformed filters of the 64 -> 64 3x3 layers (wino3.hip), which the separate wino3_pack_k launch wrote behind the operands,
// are computed by further workgroups of this launch from the same canonical weights (blocks from wino_first on, 16 per layer).
constexpr int kPackTc = 9, kPackRow = 32 * kPackTc + 1;
struct PackBatchWide {
    PackBatch b;                    // first[] counts this kernel's blocks: cdiv(Cin, 32) * cdiv(Cout, 32) * chunks per layer
    unsigned long long wino_mask;   // bit e: layer e also gets the fused-Winograd filters behind wf / wb
    int wino_first;                 // first of the workgroups that compute those
};
__host__ __device__ static inline int pack_chunks(int KK) { return (KK + (KK <= kPackTc ? kPackTc : 8) - 1) / (KK <= kPackTc ? kPackTc : 8); }
__global__ __launch_bounds__(256) void pack_weight_batch_wide_kernel(PackBatchWide a) {
    __shared__ float sh[32 * kPackRow];
    const PackBatch& b = a.b;
    if ((int)blockIdx.x >= a.wino_first) {
        const int r = (int)blockIdx.x - a.wino_first;
        int e = 0;
        for (int job = r / 16; e < b.n; ++e)
            if (((a.wino_mask >> e) & 1ull) && job-- == 0) break;
        if (e < b.n)
            cg::wino3_pack_item(b.w[e], b.wf[e] ? b.wf[e] + cg::kWino3UOffset : nullptr, b.wb[e] ? b.wb[e] + cg::kWino3UOffset : nullptr,
                                (r % 16) * 256 + (int)threadIdx.x);
        return;
    }
    int e = 0;
    while (e + 1 < b.n && (int)blockIdx.x >= b.first[e + 1]) ++e;
    const float* w = b.w[e]; float* wf = b.wf[e]; float* wb = b.wb[e];
    const int Cout = b.Cout[e], Cin = b.Cin[e], KK = b.KK[e];
    const bool wb_map = (b.map_mask >> e) & 1ull;
    const int nbx = (Cin + 31) / 32, nby = (Cout + 31) / 32, nch = pack_chunks(KK);
    const int tc = (KK + nch - 1) / nch;                 // taps per chunk (the last chunk may hold fewer)
    int r = (int)blockIdx.x - b.first[e];
    const int bx = r % nbx; r /= nbx;
    const int by = r % nby;
    const int tap0 = (r / nby) * tc, nt = min(tc, KK - tap0);
    const int ci0 = bx * 32, co0 = by * 32;
    if (KK == 1) {      // linear / 1 x 1 layers: the canonical rows are read coalesced as they are, nothing to stage
        pack_block_tap(*reinterpret_cast<float (*)[32][33]>(sh), w, wf, wb, Cout, Cin, 1, wb_map, ci0, co0, 0);
        return;
    }
    // stage: wave v takes the block's rows co_l = v, v + 4, ...; a row is 32 runs of nt floats, KK floats apart
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        constexpr int SLOTS = (32 * kPackTc + 63) / 64;
        int goff[SLOTS], loff[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int el = lane + 64 * s, ci_l = el / nt, tt = el - ci_l * nt;
            const bool ok = ci_l < 32 && ci0 + ci_l < Cin;
            goff[s] = ok ? ci_l * KK + tt : -1;
            loff[s] = ci_l * kPackTc + tt;
        }
#pragma unroll 2
        for (int co_l = wave; co_l < 32 && co0 + co_l < Cout; co_l += 4) {
            const float* src = w + ((long)(co0 + co_l) * Cin + ci0) * KK + tap0;
            float v[SLOTS];      // every slot loads (an idle one the row's first float), so that the loads are issued together
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) v[s] = src[max(goff[s], 0)];
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (goff[s] >= 0) sh[co_l * kPackRow + loff[s]] = v[s];
        }
    }
    __syncthreads();
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    if (wb && ci0 + lo < Cin) {
        const int ci = ci0 + lo;
        for (int tt = 0; tt < nt; ++tt) {
            const int tap = tap0 + tt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co_l = hi + 8 * j, co = co0 + co_l;
                if (co < Cout)
                    wb[wb_map ? ((long)co * KK + tap) * Cin + ci : ((long)(KK - 1 - tap) * Cout + co) * Cin + ci] = sh[co_l * kPackRow + lo * kPackTc + tt];
            }
        }
    }
    if (wf && co0 + lo < Cout) {
        const int co = co0 + lo;
        for (int tt = 0; tt < nt; ++tt) {
            const int tap = tap0 + tt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ci_l = hi + 8 * j, ci = ci0 + ci_l;
                if (ci < Cin) wf[((long)tap * Cin + ci) * Cout + co] = sh[lo * kPackRow + ci_l * kPackTc + tt];
            }
        }
    }
}

// upsample(2) -> conv K x K, K in {3, 5} (the generator's layers): KP = KPD x KPD low-res taps per phase
template <int K>
struct Ups2 { static constexpr int KK = K * K, PAD = (K - 1) / 2, KPD = K == 3 ? 2 : 3, KP = KPD * KPD; };
// The taps of phase P = 2a + b of one (co, ci): acc[t'] = the sum of the canonical taps v[dy][dx] that fold onto low-res tap t', added from
// 0.f in (dy, dx) order - the order the two kernels below promise each other.  Every accumulator index is a compile-time constant.
template <int K, int P>
__device__ __forceinline__ void phase_sums(const float (&v)[Ups2<K>::KK], float (&acc)[Ups2<K>::KP]) {
    using U = Ups2<K>;
#pragma unroll
    for (int t = 0; t < U::KP; ++t) acc[t] = 0.f;
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) acc[phase_map(P >> 1, dy, U::PAD) * U::KPD + phase_map(P & 1, dx, U::PAD)] += v[dy * K + dx];
}

// phase-summed weights: same 32x32 blocking as pack_weight_kernel, a thread walks the four phases of its four (co, ci) in turn
template <int K, int P>
__device__ __forceinline__ void pack_ups2_fast_phase(float (&sh)[Ups2<K>::KP][32][33], const float (&v)[4][Ups2<K>::KK], float* wf, float* wb,
                                                     int Cout, int Cin, int ci0, int co0) {
    constexpr int KP = Ups2<K>::KP;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float acc[KP];
        phase_sums<K, P>(v[j], acc);
        const int ci = ci0 + lo, co_l = hi + 8 * j, co = co0 + co_l;
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            if (wb && ci < Cin && co < Cout) wb[(((long)P * KP + t) * Cout + co) * Cin + ci] = acc[t];
            sh[t][lo][co_l] = acc[t];
        }
    }
    if (wf) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < KP; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + lo, ci_l = hi + 8 * j, ci = ci0 + ci_l;
                if (ci < Cin && co < Cout) wf[(((long)P * KP + t) * Cin + ci) * Cout + co] = sh[t][ci_l][lo];
            }
        __syncthreads();
    }
}
template <int K>
__global__ __launch_bounds__(256) void pack_weight_ups2_fast_kernel(const float* w, float* wf, float* wb, int Cout, int Cin) {
    constexpr int KK = Ups2<K>::KK;
    __shared__ float sh[Ups2<K>::KP][32][33];
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    float v[4][KK];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + lo, co = co0 + hi + 8 * j;
        const bool ok = ci < Cin && co < Cout;
        const float* src = w + ((long)co * Cin + ci) * KK;
#pragma unroll
        for (int t = 0; t < KK; ++t) v[j][t] = ok ? src[t] : 0.f;
    }
    pack_ups2_fast_phase<K, 0>(sh, v, wf, wb, Cout, Cin, ci0, co0);
    pack_ups2_fast_phase<K, 1>(sh, v, wf, wb, Cout, Cin, ci0, co0);
    pack_ups2_fast_phase<K, 2>(sh, v, wf, wb, Cout, Cin, ci0, co0);
    pack_ups2_fast_phase<K, 3>(sh, v, wf, wb, Cout, Cin, ci0, co0);
}

// The wide form of the same (CG_PACK_WIDE, the default): one workgroup owns ONE phase of a 32 ci x kPackWideCo co block, so the
// launch has 4 * 32 / kPackWideCo times the workgroups of the kernel above (G32up's 256 -> 128 5x5 layer: 256 instead of 32, its
// 512 -> 256 3x3 layer: 1024 instead of 128) and no thread walks the four phases in turn.  The canonical taps of a co row of the
// block are 32 * K * K contiguous floats: they are read coalesced into LDS, and every thread then takes its own K * K taps from there
// (lane stride K * K words, odd: no bank conflicts).  Each phase tap comes out of the same phase_sums, so the bits are those of the
// kernel above; wb is stored ci-fastest straight from the registers, wf
// co-fastest through an LDS transpose that reuses the staging area.
constexpr int kPackWideCo = 16;
template <int K, int P>
__device__ __forceinline__ void pack_ups2_wide_phase(float* sh, float* wf, float* wb, int Cout, int Cin, int ci0, int co0) {
    constexpr int KK = Ups2<K>::KK, KP = Ups2<K>::KP, RUN = 32 * KK, J = kPackWideCo / 8;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int ci = ci0 + lo;
    float acc[J][KP];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const float* src = sh + (hi + 8 * j) * RUN + lo * KK;
        float v[KK];
#pragma unroll
        for (int t = 0; t < KK; ++t) v[t] = src[t];
        phase_sums<K, P>(v, acc[j]);
        const int co = co0 + hi + 8 * j;
        if (wb && ci < Cin && co < Cout) {
#pragma unroll
            for (int t = 0; t < KP; ++t) wb[(((long)P * KP + t) * Cout + co) * Cin + ci] = acc[j][t];
        }
    }
    if (wf) {
        constexpr int LD = kPackWideCo + 1;
        __syncthreads();      // every thread has its taps in registers: the staging area becomes the [KP][32][LD] transpose buffer
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int t = 0; t < KP; ++t) sh[(t * 32 + lo) * LD + hi + 8 * j] = acc[j][t];
        __syncthreads();
        const int co_l = threadIdx.x % kPackWideCo, co = co0 + co_l;
#pragma unroll
        for (int t = 0; t < KP; ++t)
            for (int ci_l = threadIdx.x / kPackWideCo; ci_l < 32; ci_l += 256 / kPackWideCo)
                if (ci0 + ci_l < Cin && co < Cout) wf[(((long)P * KP + t) * Cin + ci0 + ci_l) * Cout + co] = sh[(t * 32 + ci_l) * LD + co_l];
    }
}
template <int K>
__global__ __launch_bounds__(256) void pack_weight_ups2_wide_kernel(const float* w, float* wf, float* wb, int Cout, int Cin) {
    constexpr int KK = K * K, RUN = 32 * KK;
    static_assert(kPackWideCo % 8 == 0 && 256 % kPackWideCo == 0 && (K == 3 ? 4 : 9) * 32 * (kPackWideCo + 1) <= kPackWideCo * RUN,
                  "the transpose buffer lies inside the staging area");
    __shared__ float sh[kPackWideCo * RUN];
    const int ci0 = blockIdx.x * 32, co0 = (blockIdx.y / 4) * kPackWideCo, p = blockIdx.y & 3;
    const int run = min(32, Cin - ci0) * KK;      // floats of a co row that belong to this block
    for (int idx = threadIdx.x; idx < kPackWideCo * RUN; idx += 256) {
        const int co_l = idx / RUN, j = idx - co_l * RUN;
        sh[idx] = co0 + co_l < Cout && j < run ? w[((long)(co0 + co_l) * Cin + ci0) * KK + j] : 0.f;
    }
    __syncthreads();
    switch (p) {      // the phase as a template argument: every accumulator index is a compile-time constant
        case 0: pack_ups2_wide_phase<K, 0>(sh, wf, wb, Cout, Cin, ci0, co0); break;
        case 1: pack_ups2_wide_phase<K, 1>(sh, wf, wb, Cout, Cin, ci0, co0); break;
        case 2: pack_ups2_wide_phase<K, 2>(sh, wf, wb, Cout, Cin, ci0, co0); break;
        default: pack_ups2_wide_phase<K, 3>(sh, wf, wb, Cout, Cin, ci0, co0); break;
    }
}

// phase-summed weights for upsample(2) -> conv k x k:
//   wf[p][(t'*Cin+ci)][co] = sum_{(dy,dx) -> t' under phase p} w[co][ci][dy][dx]
//   wb[((p*kp*kp + t')*Cout + co)][ci] = the same value (data-gradient operand)
// Same LDS staging as pack_weight_kernel.
__global__ __launch_bounds__(256) void pack_weight_ups2_kernel(const float* w, float* wf, float* wb, int Cout, int Cin, int k,
                                                               int pad, int kp, int CI_T) {
    extern __shared__ float sh[];  // [32][CI_T*KK + 1]
    const int KK = k * k, KP = kp * kp;
    const int run = CI_T * KK, ld = run + 1;
    const int ci0 = blockIdx.x * CI_T, co0 = blockIdx.y * 32;
    const int cis = min(CI_T, Cin - ci0);
    for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
        const int j = idx % run, co_l = idx / run;
        if (co0 + co_l < Cout && j < cis * KK) sh[co_l * ld + j] = w[((long)(co0 + co_l) * Cin + ci0) * KK + j];
    }
    __syncthreads();
    const int n = 4 * KP * CI_T * 32;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? wf == nullptr : wb == nullptr) continue;
        for (int idx = threadIdx.x; idx < n; idx += 256) {
            int co_l, ci_l, q;
            if (pass == 0) { co_l = idx & 31; const int r = idx >> 5; ci_l = r % CI_T; q = r / CI_T; }
            else { ci_l = idx % CI_T; const int r = idx / CI_T; co_l = r & 31; q = r >> 5; }
            if (co0 + co_l >= Cout || ci_l >= cis) continue;
            const int tp = q % KP, p = q / KP;
            const int ry = tp / kp, rx = tp - ry * kp;
            const float* src = sh + co_l * ld + ci_l * KK;
            float s = 0.f;
            for (int dy = 0; dy < k; ++dy) {
                if (phase_map(p >> 1, dy, pad) != ry) continue;
                for (int dx = 0; dx < k; ++dx)
                    if (phase_map(p & 1, dx, pad) == rx) s += src[dy * k + dx];
            }
            if (pass == 0) wf[(((long)p * KP + tp) * Cin + ci0 + ci_l) * Cout + co0 + co_l] = s;
            else wb[(((long)p * KP + tp) * Cout + co0 + co_l) * Cin + ci0 + ci_l] = s;
        }
    }
}

}  // namespace

extern "C" {

// input channels per pack workgroup: the largest power of two with ci_t*KK <= 448 floats per output channel (57 KB of LDS)
static int pack_ci_tile(int Cin, int KK) {
    int t = 1;
    while (t * 2 * KK <= 448 && t < Cin) t *= 2;
    return t;
}

int cg_pack_conv_weight(void* stream, const float* w, float* wf, float* wb, int Cout, int Cin, int kH, int kW) {
    CG_REQUIRE(w && (wf || wb), "cg_pack_conv_weight: null pointer");
    CG_REQUIRE(Cout > 0 && Cin > 0 && kH > 0 && kW > 0, "cg_pack_conv_weight: bad dims");
    const int KK = kH * kW;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(cg::cdiv(Cin, 32), cg::cdiv(Cout, 32), KK), dim3(256), 0, cg::S(stream), w,
                       wf, wb, Cout, Cin, KK, 0);
    CG_LAUNCH_CHECK();
    return cg::wino3_note_pack(cg::S(stream), 1, &w, &wf, &wb, &Cout, &Cin, &kH, &kW, nullptr);
}

// nn.View(C*H*W) -> nn.Linear(C*H*W -> Cout) on an NHWC map (models.lua:696-697, 849-850) without materialising the NCHW
// view: the canonical [Cout][C*H*W] weight IS the canonical weight of a convolution C -> Cout with an H x W kernel, no
// padding, on the H x W map (output 1 x 1).  wf (forward / weight-gradient view) is cg_pack_conv_weight's;
// wbT[co][(h*W+w)*C + c] = w[co][c][h][w] is the [K = Cout][N = H*W*C] operand of the data gradient, run as a linear layer:
//   cg_conv2d_forward(dy [N][Cout], wbT, NULL, dx [N][H*W*C] = NHWC, N, 1, 1, Cout, H*W*C, 1, 1, 0, 0, 0)
int cg_pack_conv_weight_map(void* stream, const float* w, float* wf, float* wbT, int Cout, int Cin, int kH, int kW) {
    CG_REQUIRE(w && (wf || wbT), "cg_pack_conv_weight_map: null pointer");
    CG_REQUIRE(Cout > 0 && Cin > 0 && kH > 0 && kW > 0, "cg_pack_conv_weight_map: bad dims");
    const int KK = kH * kW;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(cg::cdiv(Cin, 32), cg::cdiv(Cout, 32), KK), dim3(256), 0, cg::S(stream), w,
                       wf, wbT, Cout, Cin, KK, 1);
    CG_LAUNCH_CHECK();
    return 0;
}

int cg_pack_conv_weight_batch(void* stream, int n, const float* const* w_canonical, float* const* wf, float* const* wb,
                              const int* Cout, const int* Cin, const int* kH, const int* kW, const int* wb_map) {
    CG_REQUIRE(n >= 0 && w_canonical && wf && wb && Cout && Cin && kH && kW, "cg_pack_conv_weight_batch: null pointer");
    const bool wide = cg::opt(cg::OPT_PACK_WIDE) != 0;
    for (int i0 = 0; i0 < n; i0 += kPackBatch) {
        // one chunk of layers; the two kernels differ in the blocks of a 32 x 32 (ci, co) block: one per tap chunk (wide) or per tap
        PackBatchWide a;
        memset(&a, 0, sizeof(a));
        PackBatch& b = a.b;
        b.n = std::min(kPackBatch, n - i0);
        int blocks = 0, wino = 0;
        for (int e = 0; e < b.n; ++e) {
            const int i = i0 + e;
            CG_REQUIRE(w_canonical[i] && (wf[i] || wb[i]) && Cout[i] > 0 && Cin[i] > 0 && kH[i] > 0 && kW[i] > 0,
                       "cg_pack_conv_weight_batch: bad layer %d", i);
            b.w[e] = w_canonical[i]; b.wf[e] = wf[i]; b.wb[e] = wb[i];
            b.Cout[e] = Cout[i]; b.Cin[e] = Cin[i]; b.KK[e] = kH[i] * kW[i];
            const bool map = wb_map && wb_map[i];
            if (map) b.map_mask |= 1ull << e;
            if (cg::wino3_layer(Cout[i], Cin[i], kH[i], kW[i]) && !map) { a.wino_mask |= 1ull << e; ++wino; }      // wino3_note_pack's rule
            b.first[e] = blocks;
            blocks += cg::cdiv(Cin[i], 32) * cg::cdiv(Cout[i], 32) * (wide ? pack_chunks(b.KK[e]) : b.KK[e]);
        }
        b.first[b.n] = blocks;
        a.wino_first = blocks;
        // the wide launch computes the fused-Winograd filters itself, in 16 further workgroups per such layer
        if (wide) hipLaunchKernelGGL(pack_weight_batch_wide_kernel, dim3(blocks + 16 * wino), dim3(256), 0, cg::S(stream), a);
        else hipLaunchKernelGGL(pack_weight_batch_kernel, dim3(blocks), dim3(256), 0, cg::S(stream), b);
        CG_LAUNCH_CHECK();
    }
    return wide ? 0 : cg::wino3_note_pack(cg::S(stream), n, w_canonical, wf, wb, Cout, Cin, kH, kW, wb_map);
}

size_t cg_pack_conv_weight_floats(int Cout, int Cin, int kH, int kW) {
    if (Cout <= 0 || Cin <= 0 || kH <= 0 || kW <= 0) return 0;
    return (size_t)kH * kW * Cin * Cout + (cg::wino3_layer(Cout, Cin, kH, kW) ? cg::kWino3UFloats : 0);
}

size_t cg_pack_conv_weight_ups2_floats(int Cout, int Cin, int k, int pad) {
    if (Cout <= 0 || Cin <= 0 || k <= 0 || (k & 1) == 0 || pad != (k - 1) / 2) return 0;
    const int kp = phase_kp(k, pad);
    return (size_t)4 * kp * kp * Cin * Cout;
}

int cg_pack_conv_weight_ups2(void* stream, const float* w, float* wf_ph, float* wb_ph, int Cout, int Cin, int k, int pad) {
    CG_REQUIRE(w && (wf_ph || wb_ph), "cg_pack_conv_weight_ups2: null pointer");
    CG_REQUIRE(Cout > 0 && Cin > 0 && k > 0 && (k & 1) == 1 && pad == (k - 1) / 2,
               "cg_pack_conv_weight_ups2: needs an odd kernel with pad=(k-1)/2");
    const int kp = phase_kp(k, pad);
    CG_REQUIRE(k * k <= 448, "cg_pack_conv_weight_ups2: kernel too large (%d taps)", k * k);
    const dim3 fgrid(cg::cdiv(Cin, 32), cg::cdiv(Cout, 32));
    if ((k == 3 || k == 5) && cg::opt(cg::OPT_PACK_WIDE) != 0) {
        const dim3 wgrid(cg::cdiv(Cin, 32), cg::cdiv(Cout, kPackWideCo) * 4);
        hipLaunchKernelGGL(k == 3 ? pack_weight_ups2_wide_kernel<3> : pack_weight_ups2_wide_kernel<5>, wgrid, dim3(256), 0, cg::S(stream), w, wf_ph,
                           wb_ph, Cout, Cin);
        CG_LAUNCH_CHECK();
        return 0;
    }
    if (k == 3 || k == 5) {
        hipLaunchKernelGGL(k == 3 ? pack_weight_ups2_fast_kernel<3> : pack_weight_ups2_fast_kernel<5>, fgrid, dim3(256), 0, cg::S(stream), w, wf_ph,
                           wb_ph, Cout, Cin);
        CG_LAUNCH_CHECK();
        return 0;
    }
    const int ci_t = pack_ci_tile(Cin, k * k);
    hipLaunchKernelGGL(pack_weight_ups2_kernel, dim3(cg::cdiv(Cin, ci_t), cg::cdiv(Cout, 32)), dim3(256),
                       (size_t)32 * (ci_t * k * k + 1) * sizeof(float), cg::S(stream), w, wf_ph, wb_ph, Cout, Cin, k, pad, kp,
                       ci_t);
    CG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
