// Winograd F(2x2,3x3) for nn.SpatialUpSamplingNearest(2) -> 5x5 convolution (models.lua:217-218, G's
// 256 -> 128 layer: 60 % of the generator's FLOPs).
//
// After the phase folding of gemm.hip, output phase (a,b) of that layer is a plain 3x3 / pad-1 convolution of the
// LOW-RESOLUTION input with the phase-summed kernel g_p (both phases of a 5-tap axis reach rows i-1..i+1).  All
// four phases therefore share their 4x4 input tiles, and each is computed as
//     Y_p = A^T [ (G g_p G^T) .* (B^T d B) ] A            (Lavin & Gray, F(2x2,3x3): 16 multiplies per 4 outputs
// instead of 36, i.e. 2.25x fewer MFMA FLOPs on top of the 2.78x of the phase folding)
// as 16 GEMMs  M_xi[tile][co] = sum_ci V_xi[tile][ci] U_p,xi[ci][co]  whose output transform happens in registers:
// one workgroup walks xi = 0..15 for its (tile block, co block, phase), folding every finished M_xi into the four
// output accumulators with the +-1/0 coefficients of A^T (x) A^T.  Nothing Winograd-domain but V is ever written.
//
// The data gradient w.r.t. the low-res input is the same machinery on dy: one 3x3 convolution with 4*Cout input
// planes (the four phase sub-lattices of dy) and flipped kernels.  The weight gradient is taken in the Winograd
// domain (dU_xi = V_xi^T (A dY A^T)_xi, 16 plain TN GEMMs through cg_conv2d_wgrad) and brought back by G^T . G.
//
// F(2x2,2x2) for upsample -> 3x3 convolution (models.lua:211-212) is the same with 2x2 phase kernels and 9 positions.
// What the two families and their kernels share lives once:
//   transforms : wino_tile_walk (the (tile, channel quad) walk of all five input-side kernels), wino_load_patch (4x4 patch of a plain
//                tensor) and wino_load_dy_patch<side, origin> (a patch of dy's phase sub-lattices); a kernel adds its own B^T . B or A . A^T
//   filters    : wino_filter_transform_items / _kernel / _both_kernel<Family>; WinoF23 and WinoF22 supply the tap count and G g G^T
//   GEMMs      : wino_place (XCD placement), wino_out_coeffs<NPOS> (A^T (x) A^T), wino_store_generic + wino_store_stats (the generic
//                store-and-statistics tail) under wino_gemm_kernel (register staging) and wino_gemm_g_kernel (LDS-direct loads)
//   host       : glds_ok, wino_gemm_launch, wino_pack<Family>, wino_dgrad_pair (transform + GEMMs, K-sliced or not, of both families)
//
// Numerics: exact-fp32 MFMA as everywhere; the transforms add a few ulp (entries 0, +-1, +-1/2), the parity
// tests hold the layer to the same 2e-5*sqrt(K/1024) bound as the direct path.
#include "common.h"
#include <algorithm>
#include <type_traits>
#include <stdlib.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

using cg::ld4;
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
using cg::f4c;
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4neg(float4 a) { return make_float4(-a.x, -a.y, -a.z, -a.w); }

// ---------------------------------------------------------------------------
// Input-side transforms: one thread per (tile, channel quad), float4 loads and stores coalesced along the channels.
// ---------------------------------------------------------------------------
// The walk they share, over the 2x2 tiles of [N][Hl][Wl] and the quads of C channels: body(n, ti, tj, c, off, xs) gets the image, the
// tile's row and column, the quad's first channel, the offset of plane 0's element [tile][c] and the stride between planes.
template <class Body>
__device__ __forceinline__ void wino_tile_walk(int N, int Hl, int Wl, int C, Body body) {
    const int cq_n = C >> 2;
    const int tH = Hl >> 1, tW = Wl >> 1;
    const long T = (long)N * tH * tW;
    const long total = T * cq_n;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += gridDim.x * 256L) {
        const int cq = (int)(idx % cq_n);
        const long tile = idx / cq_n;
        const int tj = (int)(tile % tW);
        const int ti = (int)((tile / tW) % tH);
        const long n = tile / ((long)tW * tH);
        body(n, ti, tj, cq * 4, tile * C + cq * 4, T * C);
    }
}

// d = the 4x4 patch around tile (n, ti, tj), rows 2ti-1 .. 2ti+2, of a plain NHWC tensor [N][Hl][Wl][C]: zero outside the image
__device__ __forceinline__ void wino_load_patch(const float* src, long n, int ti, int tj, int Hl, int Wl, int C, int c, float4 (&d)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int iy = 2 * ti - 1 + r, ix = 2 * tj - 1 + cc;
            const bool ok = iy >= 0 && iy < Hl && ix >= 0 && ix < Wl;
            const int cy = min(max(iy, 0), Hl - 1), cx = min(max(ix, 0), Wl - 1);
            const float4 q = ld4(src + ((n * Hl + cy) * (long)Wl + cx) * C + c);
            d[r][cc] = ok ? q : make_float4(0.f, 0.f, 0.f, 0.f);
        }
}

// The same of the phase sub-lattices of dy [N][2Hl][2Wl][Cs]: channel c = p*Cs + co reads dy[2i+a][2j+b][co], (a, b) = phase p.
// S x S pixels from row 2ti - 1 (BY_PHASE false: F(2x2,3x3)) or from row 2ti - a (true: the window of F(2x2,2x2)'s data gradient).
template <int S, bool BY_PHASE>
__device__ __forceinline__ void wino_load_dy_patch(const float* dy, long n, int ti, int tj, int Hl, int Wl, int Cs, int c, float4 (&d)[S][S]) {
    const int p = c / Cs, cs = c - p * Cs;
    const int pa = p >> 1, pb = p & 1;
#pragma unroll
    for (int r = 0; r < S; ++r)
#pragma unroll
        for (int cc = 0; cc < S; ++cc) {
            const int iy = 2 * ti - (BY_PHASE ? pa : 1) + r, ix = 2 * tj - (BY_PHASE ? pb : 1) + cc;
            const bool ok = iy >= 0 && iy < Hl && ix >= 0 && ix < Wl;
            const int cy = min(max(iy, 0), Hl - 1), cx = min(max(ix, 0), Wl - 1);
            const float4 q = ld4(dy + ((n * 2 * Hl + 2 * cy + pa) * (long)(2 * Wl) + 2 * cx + pb) * Cs + cs);
            d[r][cc] = ok ? q : make_float4(0.f, 0.f, 0.f, 0.f);
        }
}

// F(2x2,3x3): V[xi][tile][c] = (B^T d B)[xi] of the 4x4 patch.  MODE 0: d from a plain tensor; MODE 1: from dy's sub-lattices (C = 4 Cs).
template <int MODE>
__global__ __launch_bounds__(256) void wino_input_transform_kernel(const float* __restrict__ src, float* __restrict__ V,
                                                                   int N, int Hl, int Wl, int C, int Cs) {
    wino_tile_walk(N, Hl, Wl, C, [&](long n, int ti, int tj, int c0, long off, long xs) {
        float4 d[4][4];
        if (MODE == 0) wino_load_patch(src, n, ti, tj, Hl, Wl, C, c0, d);
        else wino_load_dy_patch<4, false>(src, n, ti, tj, Hl, Wl, Cs, c0, d);
        float4 t[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // B^T d
            t[0][c] = f4sub(d[0][c], d[2][c]);
            t[1][c] = f4add(d[1][c], d[2][c]);
            t[2][c] = f4sub(d[2][c], d[1][c]);
            t[3][c] = f4sub(d[1][c], d[3][c]);
        }
        float* out = V + off;
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // (.) B
            st4(out + (r * 4 + 0) * xs, f4sub(t[r][0], t[r][2]));
            st4(out + (r * 4 + 1) * xs, f4add(t[r][1], t[r][2]));
            st4(out + (r * 4 + 2) * xs, f4sub(t[r][2], t[r][1]));
            st4(out + (r * 4 + 3) * xs, f4sub(t[r][1], t[r][3]));
        }
    });
}

// F(2x2,2x2) for nn.SpatialUpSamplingNearest(2) -> 3x3 convolution (models.lua:211-212; round 4).  After the phase folding, output
// phase (a,b) is a 2x2-tap convolution of the low-res input whose window starts at row -1 + a, column -1 + b: per 2x2 tile of low-res
// outputs and phase, 16 multiplies per channel pair; Winograd's minimal form needs 9 (y0 = (d0-d1) g0 + d1 (g0+g1), y1 = d1 (g0+g1) +
// (d2-d1) g1 per axis: B^T = [1 -1 0; 0 1 0; 0 -1 1], G = [1 0; 1 1; 0 1], A^T = [1 1 0; 0 1 1] - all 0 / +-1, exact up to the
// additions).  The four phases' 3x3 windows are the four 3x3 corners of ONE 4x4 patch (rows 2ti-1 .. 2ti+2), so the input transform
// reads the patch once and writes 4 x 9 planes:  V[(p*9 + xi)][tile][c].  The GEMMs and the output transform are wino_gemm_g_kernel's
// with 9 positions and V taken per phase.
__global__ __launch_bounds__(256) void wino22_input_transform_kernel(const float* __restrict__ src, float* __restrict__ V, int N, int Hl,
                                                                     int Wl, int C) {
    wino_tile_walk(N, Hl, Wl, C, [&](long n, int ti, int tj, int c0, long off, long xs) {
        float4 d[4][4];
        wino_load_patch(src, n, ti, tj, Hl, Wl, C, c0, d);
        float* out = V + off;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float4 t[3][4];   // B^T applied to rows a .. a+2, all four columns
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                t[0][c] = f4sub(d[a][c], d[a + 1][c]);
                t[1][c] = d[a + 1][c];
                t[2][c] = f4sub(d[a + 2][c], d[a + 1][c]);
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const long pbase = (long)(a * 2 + b) * 9;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    st4(out + (pbase + i * 3 + 0) * xs, f4sub(t[i][b], t[i][b + 1]));
                    st4(out + (pbase + i * 3 + 1) * xs, t[i][b + 1]);
                    st4(out + (pbase + i * 3 + 2) * xs, f4sub(t[i][b + 2], t[i][b + 1]));
                }
            }
        }
    });
}

// Data gradient of the same layers.  dx_lo[u][v] = sum_p sum_r dy_p[u - a + ry][v - b + rx] . g_p[1-ry][1-rx] over the phase
// sub-lattices dy_p[i][j] = dy[2i+a][2j+b]: per phase a 2x2-tap correlation with the flipped kernel whose window starts at row u - a,
// the four phases summed - one F(2x2,2x2) problem with the phases side by side along K (K = 4 Cout).
// V[xi][tile][p*Cs + co] = B^T d B of the 3x3 patch (rows 2ti - a .. 2ti - a + 2 of sub-lattice p).
__global__ __launch_bounds__(256) void wino22_dy_input_transform_kernel(const float* __restrict__ dy, float* __restrict__ V, int N, int Hl,
                                                                        int Wl, int Cs) {
    wino_tile_walk(N, Hl, Wl, 4 * Cs, [&](long n, int ti, int tj, int c0, long off, long xs) {
        float4 d[3][3];
        wino_load_dy_patch<3, true>(dy, n, ti, tj, Hl, Wl, Cs, c0, d);
        float4 t[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { t[0][c] = f4sub(d[0][c], d[1][c]); t[1][c] = d[1][c]; t[2][c] = f4sub(d[2][c], d[1][c]); }
        float* out = V + off;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            st4(out + (i * 3 + 0) * xs, f4sub(t[i][0], t[i][1]));
            st4(out + (i * 3 + 1) * xs, t[i][1]);
            st4(out + (i * 3 + 2) * xs, f4sub(t[i][2], t[i][1]));
        }
    });
}

// Weight gradient of F(2x2,3x3), Winograd domain: Mdy[xi][tile][p*Cout+co] = (A dY_p A^T)[xi] per tile and phase (A = [1 0; 1 1; 1 -1;
// 0 -1]); then dU_xi = V_xi^T Mdy_xi (plain TN GEMMs) and wino_wgrad_finish_kernel maps G^T dU G back to the 5x5 taps.
// (gradBias partial sums from this kernel - it reads every dy anyway - were parity-clean but cost the step 0.6 % in round 4: the separate
// 59 us pass of cg_bias_grad is not on the critical path, the longer transform is.)
__global__ __launch_bounds__(256) void wino_dy_transform_kernel(const float* __restrict__ dy, float* __restrict__ Mdy, int N,
                                                                int Hl, int Wl, int Cout) {
    wino_tile_walk(N, Hl, Wl, 4 * Cout, [&](long n, int ti, int tj, int c0, long off, long xs) {
        const int p = c0 / Cout, co = c0 - p * Cout;
        const int pa = p >> 1, pb = p & 1;
        float4 e[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
                e[u][v] = ld4(dy + ((n * 2 * Hl + 2 * (2 * ti + u) + pa) * (long)(2 * Wl) + 2 * (2 * tj + v) + pb) * Cout + co);
        float4 r[4][2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            r[0][v] = e[0][v];
            r[1][v] = f4add(e[0][v], e[1][v]);
            r[2][v] = f4sub(e[0][v], e[1][v]);
            r[3][v] = f4neg(e[1][v]);
        }
        float* out = Mdy + off;
#pragma unroll
        for (int xy = 0; xy < 4; ++xy) {
            st4(out + (xy * 4 + 0) * xs, r[xy][0]);
            st4(out + (xy * 4 + 1) * xs, f4add(r[xy][0], r[xy][1]));
            st4(out + (xy * 4 + 2) * xs, f4sub(r[xy][0], r[xy][1]));
            st4(out + (xy * 4 + 3) * xs, f4neg(r[xy][1]));
        }
    });
}

// out = the sum of S (2 or 4) partial results `stride` floats apart, in a fixed order: the K slices of a sliced data gradient
template <int S>
__global__ __launch_bounds__(256) void wino22_sum_kernel(const float* __restrict__ part, float* __restrict__ out, long n4, long stride) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
        const float4 a = ld4(part + 4 * i), b = ld4(part + stride + 4 * i);
        float4 r = f4add(a, b);
        if (S == 4) r = f4add(r, f4add(ld4(part + 2 * stride + 4 * i), ld4(part + 3 * stride + 4 * i)));
        st4(out + 4 * i, r);
    }
}

// ---------------------------------------------------------------------------
// U = G g G^T of the phase kernels, R x R taps -> P x P positions.
// FWD: src = wf_ph [p][tp][ci][co]  ->  U[p][xi][ci][co]
// BWD: src = wb_ph [p][tp][co][ci]  ->  U[xi][p*Cout+co][ci] of the FLIPPED kernel (data gradient operand: the four phases side by side
//      along K)
// One thread per (p, row, column quad) of the [rows][cols] plane (rows x cols = Cin x Cout or Cout x Cin).  A family supplies its tap
// count, its position count and G g G^T on float4s; the walk, the flip and the destination index are the same for both.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float4 f4half_sum(float4 s, float4 g) {   // 0.5 (s + g)
    return make_float4(0.5f * (s.x + g.x), 0.5f * (s.y + g.y), 0.5f * (s.z + g.z), 0.5f * (s.w + g.w));
}
__device__ __forceinline__ float4 f4half_diff(float4 s, float4 g) {  // 0.5 (s - g)
    return make_float4(0.5f * (s.x - g.x), 0.5f * (s.y - g.y), 0.5f * (s.z - g.z), 0.5f * (s.w - g.w));
}
struct WinoF23 {   // 3x3 phase kernels of the 5x5 layer, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
    static constexpr int R = 3, P = 4;
    static __device__ __forceinline__ void ggt(const float4 (&g)[3][3], float4 (&o)[16]) {
        float4 t[4][3];  // G g
#pragma unroll
        for (int rx = 0; rx < 3; ++rx) {
            const float4 s = f4add(g[0][rx], g[2][rx]);
            t[0][rx] = g[0][rx];
            t[1][rx] = f4half_sum(s, g[1][rx]);
            t[2][rx] = f4half_diff(s, g[1][rx]);
            t[3][rx] = g[2][rx];
        }
#pragma unroll
        for (int xy = 0; xy < 4; ++xy) {
            const float4 s = f4add(t[xy][0], t[xy][2]);
            o[xy * 4 + 0] = t[xy][0];
            o[xy * 4 + 1] = f4half_sum(s, t[xy][1]);
            o[xy * 4 + 2] = f4half_diff(s, t[xy][1]);
            o[xy * 4 + 3] = t[xy][2];
        }
    }
};
struct WinoF22 {   // 2x2 phase kernels of the 3x3 layer, G = [1 0; 1 1; 0 1]
    static constexpr int R = 2, P = 3;
    static __device__ __forceinline__ void ggt(const float4 (&g)[2][2], float4 (&o)[9]) {
        float4 t[3][2];  // G g
#pragma unroll
        for (int rx = 0; rx < 2; ++rx) { t[0][rx] = g[0][rx]; t[1][rx] = f4add(g[0][rx], g[1][rx]); t[2][rx] = g[1][rx]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[i * 3 + 0] = t[i][0]; o[i * 3 + 1] = f4add(t[i][0], t[i][1]); o[i * 3 + 2] = t[i][1]; }
    }
};
// Items first, first + step, ... of the plane: the two kernels below differ only in which workgroups walk which operand.
template <class F, bool BWD>
__device__ __forceinline__ void wino_filter_transform_items(const float* __restrict__ src, float* __restrict__ U, int rows, int cols,
                                                            long first, long step) {
    constexpr int R = F::R, NPOS = F::P * F::P;
    const int cqn = cols >> 2;
    const long plane = (long)rows * cols;
    const long total = 4L * rows * cqn;
    for (long idx = first; idx < total; idx += step) {
        const int cq = (int)(idx % cqn);
        const int row = (int)((idx / cqn) % rows);
        const int p = (int)(idx / ((long)cqn * rows));
        float4 g[R][R];
#pragma unroll
        for (int ry = 0; ry < R; ++ry)
#pragma unroll
            for (int rx = 0; rx < R; ++rx) {
                const int tp = BWD ? (R - 1 - ry) * R + (R - 1 - rx) : ry * R + rx;
                g[ry][rx] = ld4(src + ((long)p * (R * R) + tp) * plane + (long)row * cols + cq * 4);
            }
        float4 o[NPOS];
        F::ggt(g, o);
#pragma unroll
        for (int xi = 0; xi < NPOS; ++xi)
            st4(BWD ? U + ((long)xi * 4 * rows + (long)p * rows + row) * cols + cq * 4
                    : U + (((long)p * NPOS + xi) * rows + row) * cols + cq * 4, o[xi]);
    }
}
template <class F, bool BWD>
__global__ __launch_bounds__(256) void wino_filter_transform_kernel(const float* __restrict__ src, float* __restrict__ U,
                                                                    int rows, int cols) {
    wino_filter_transform_items<F, BWD>(src, U, rows, cols, blockIdx.x * 256L + threadIdx.x, gridDim.x * 256L);
}
// Both operands in ONE launch (CG_PACK_WIDE): workgroups [0, nf) walk the forward operand, the others the data gradient's.
template <class F>
__global__ __launch_bounds__(256) void wino_filter_transform_both_kernel(const float* __restrict__ wf_ph, float* __restrict__ u_fwd,
                                                                         const float* __restrict__ wb_ph, float* __restrict__ u_bwd,
                                                                         int Cin, int Cout, int nf) {
    const int b = blockIdx.x;
    if (b < nf) wino_filter_transform_items<F, false>(wf_ph, u_fwd, Cin, Cout, b * 256L + threadIdx.x, nf * 256L);
    else wino_filter_transform_items<F, true>(wb_ph, u_bwd, Cout, Cin, (b - nf) * 256L + threadIdx.x, ((int)gridDim.x - nf) * 256L);
}

// ---------------------------------------------------------------------------
// The 16 (or 9) GEMMs + output transform.  Block tile 64 tiles x 128 columns, 8 waves of 32 x 32.
// grid = (T/64 * Nc/128, 1, P or K slices).
// ---------------------------------------------------------------------------
struct WinoArgs {
    const float* V;      // [16][T][K]
    const float* U;      // [P][16][K][Nc]
    const float* bias;   // [Nc] or null
    float* y;            // [N][Ho][Wo][Nc]
    int T, K, Nc;
    int tH, tW;          // tiles per image
    int so;              // 2: output pixel (2i+a, 2j+b) of phase (a,b) = blockIdx.z; 1: pixel (i, j)
    int Ho, Wo;
    float* stats;        // != null: column sums of y and y^2 per (phase, tile block, wave row): [rows][2][Nc] (see gemm.hip)
    int xcd;             // XCD-aware placement of the workgroups that share a V block (CG_XCD_SWIZZLE)
    int vpp;             // 1: V holds NPOS planes PER PHASE ([P][NPOS][T][K], F(2x2,2x2)); 0: one set shared by the phases ([NPOS][T][K])
    int kz;              // > 0 (wino_gemm_g_kernel, so == 1): blockIdx.z is a K slice of kz rows, its partial result goes to y + z * T*4*Nc
    int lg_tw, lg_th;    // log2(tW), log2(tH) when both are powers of two and the output is below 2 GB (wino_gemm_g_kernel's lean epilogue), else -1
};

// Which (tile block, column block, phase) a workgroup takes.  With a.xcd the ntn * P workgroups that read the same 64-tile block of V
// (all column blocks, all phases) are placed on ONE XCD in consecutive dispatch slots, so that V comes out of that XCD's L2 after the
// first of them has fetched it (workgroup L of the dispatch order runs on XCD L % 8).  Needs a multiple of 8 tile blocks; else the
// plain (x, z) order.
struct WinoPlace { int tm, tn, phase; };
__device__ __forceinline__ WinoPlace wino_place(int xcd, int ntn) {
    int tn = blockIdx.x % ntn, tm = blockIdx.x / ntn, phase = blockIdx.z;
    const int tiles_m = gridDim.x / ntn;
    if (xcd && (tiles_m & 7) == 0) {
        const int share = ntn * (int)gridDim.z;
        const int L = (int)blockIdx.z * (int)gridDim.x + (int)blockIdx.x;
        const int slot = L >> 3, member = slot % share;
        tm = (slot / share) * 8 + (L & 7);
        phase = member / ntn;
        tn = member - phase * ntn;
    }
    return {tm, tn, phase};
}

// The coefficients (0 / +-1, wave-uniform) of a finished M_xi in a tile's four outputs (x: (0,0), y: (0,1), z: (1,0), w: (1,1)): the
// entries of A^T (x) A^T.  F(2x2,3x3), NPOS 16: A^T = [1 1 1 0; 0 1 -1 -1];  F(2x2,2x2), NPOS 9: A^T = [1 1 0; 0 1 1]
template <int NPOS>
__device__ __forceinline__ float4 wino_out_coeffs(int xi) {
    const int xy = NPOS == 16 ? xi >> 2 : xi / 3, xx = NPOS == 16 ? xi & 3 : xi - 3 * (xi / 3);
    const float cy0 = NPOS == 16 ? (xy < 3 ? 1.f : 0.f) : (xy < 2 ? 1.f : 0.f);
    const float cy1 = NPOS == 16 ? (xy == 0 ? 0.f : (xy == 1 ? 1.f : -1.f)) : (xy > 0 ? 1.f : 0.f);
    const float cx0 = NPOS == 16 ? (xx < 3 ? 1.f : 0.f) : (xx < 2 ? 1.f : 0.f);
    const float cx1 = NPOS == 16 ? (xx == 0 ? 0.f : (xx == 1 ? 1.f : -1.f)) : (xx > 0 ? 1.f : 0.f);
    return make_float4(cy0 * cx0, cy0 * cx1, cy1 * cx0, cy1 * cx1);
}

// The generic store of a wave's 32 x 32 block of the four outputs: accumulator row r holds tile mrow + (r&3) + 8*(r>>2), the lane column
// col; two integer divisions per row and a 64-bit address per value.  Returns the sums of the stored values and of their squares (stats).
// REG_STAGED keeps what differed between the two kernels when each had this tail to itself.  wino_gemm_kernel (true) sits at its 128
// registers: it re-reads the bias per value instead of holding it (bcol unused), and every square joins its sum by one fused
// multiply-add - the first two as fma(v0, v0, rn(v1 v1)), which is how 0 + v0 v0 + v1 v1 was contracted.  wino_gemm_g_kernel (false)
// holds the bias in bcol and adds the rounded square; its lean path is its own.
template <bool REG_STAGED>
__device__ __forceinline__ float2 wino_store_generic(const WinoArgs& a, float* yout, const f32x16 (&accY)[4], float bcol, int mrow, int col,
                                                     int pa, int pb) {
    float st1 = 0.f, st2 = 0.f, v0 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mrow + (r & 3) + 8 * (r >> 2);
        if (m >= a.T) continue;
        const int tj = m % a.tW;
        const int ti = (m / a.tW) % a.tH;
        const long n = m / (a.tW * a.tH);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int oy = (2 * ti + (o >> 1)) * a.so + pa, ox = (2 * tj + (o & 1)) * a.so + pb;
            const float v = accY[o][r] + (REG_STAGED ? (a.bias ? a.bias[col] : 0.f) : bcol);
            yout[((n * a.Ho + oy) * (long)a.Wo + ox) * a.Nc + col] = v;
            if (a.stats) {
                st1 += v;
                if (REG_STAGED && (r > 0 || o > 1)) st2 = __builtin_fmaf(v, v, st2);
                else {
#pragma clang fp contract(off)
                    const float sq = v * v;
                    if (!REG_STAGED) st2 += sq;
                    else if (o == 0) v0 = v;
                    else st2 = __builtin_fmaf(v0, v0, sq);
                }
            }
        }
    }
    return make_float2(st1, st2);
}
// ... and the statistics row of (phase, tile block tm, wave row wr): the two lane halves hold the two halves of the block's rows
__device__ __forceinline__ void wino_store_stats(const WinoArgs& a, int phase, int tm, int wr, int h, int col, float st1, float st2) {
    const int srow = (phase * (int)((a.T + 63) / 64) + tm) * 2 + wr;
    const float t1 = st1 + __shfl_xor(st1, 32, 64), t2 = st2 + __shfl_xor(st2, 32, 64);
    if (h == 0) {
        a.stats[((long)srow * 2 + 0) * a.Nc + col] = t1;
        a.stats[((long)srow * 2 + 1) * a.Nc + col] = t2;
    }
}

// The register-staged form (BK = K step; LDS: A [k][m] XOR-swizzled, B [k][n], double buffered, the scheme of gemm.hip): the fallback of
// wino_gemm_g_kernel below for tensors whose planes a buffer descriptor cannot span, and the reference the LDS-direct kernels are tested
// against.  (The 4-wave and k-quad instances of rounds 2-4 never won an A/B and were removed in round 5.)
template <int BK>
__global__ __launch_bounds__(512, 4) void wino_gemm_kernel(WinoArgs a) {
    constexpr int BM = 64, BN = 128, NT = 512;
    constexpr int KV = BK / 4;                 // float4 per A row per K tile
    constexpr int BQ = BK * 32 / NT;           // B float4 per thread (1 or 2), NT/32 rows apart
    static_assert(BM * KV <= NT && (BQ == 1 || BQ == 2), "staging layout");
    constexpr int A_TILE = BK * BM, B_TILE = BK * BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * A_TILE + 2 * B_TILE];
    float* As = smem;
    float* Bs = smem + 2 * A_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave & 1) * 32, wn0 = (wave >> 1) * 32;
    const WinoPlace pl = wino_place(a.xcd, a.Nc / BN);
    const int tm = pl.tm, phase = pl.phase;
    const int m0 = tm * BM, n0 = pl.tn * BN;
    const int KT = CG_PROBE_HALF(4, a.K / BK);

    // staging: A one float4 per thread (row a_r, k quad a_kv); B two float4 per thread
    const int a_kv = tid % KV, a_r = (tid / KV) % BM;
    const bool a_thr = tid < BM * KV;             // 8 waves, K step 16: the upper four waves stage only B
    const int a_row = min(m0 + a_r, a.T - 1);
    const int b_kr = tid >> 5, b_nv = tid & 31;   // k rows b_kr (and b_kr + NT/32 when BQ == 2)
    const float* Ap = a.V + (long)a_row * a.K + 4 * a_kv;
    const float* Bp = a.U + (long)phase * 16 * a.K * a.Nc + (long)b_kr * a.Nc + n0 + 4 * b_nv;
    const long a_xi = (long)a.T * a.K;            // V stride between xi
    const long b_half = (long)(NT / 32) * a.Nc;   // second B float4: k row + NT/32
    float4 areg, breg0, breg1;
    // running operand pointers: U is contiguous over (xi, k), V jumps to the next xi plane after the last K tile
    const float* Ac = Ap;
    const float* Bc = Bp;
    const long b_step = (long)BK * a.Nc;
    const long a_jump = a_xi - a.K + BK;
    auto load_next = [&](bool last_kt) {
        Ac += last_kt ? a_jump : (long)BK;
        Bc += b_step;
        if (BM * KV == NT || a_thr) areg = ld4(Ac);
        breg0 = ld4(Bc);
        if (BQ == 2) breg1 = ld4(Bc + b_half);
    };
    const int a_so = a_r ^ (BK == 32 ? ((a_kv & 7) << 2) : ((a_kv & 3) << 3));   // see a_swizzle in gemm.hip
    auto store_tile = [&](int buf) {
        float* A = As + buf * A_TILE;
        float* B = Bs + buf * B_TILE;
        if (BM * KV == NT || a_thr) {
            A[(4 * a_kv + 0) * BM + a_so] = areg.x;
            A[(4 * a_kv + 1) * BM + a_so] = areg.y;
            A[(4 * a_kv + 2) * BM + a_so] = areg.z;
            A[(4 * a_kv + 3) * BM + a_so] = areg.w;
        }
        *reinterpret_cast<float4*>(B + b_kr * BN + 4 * b_nv) = breg0;
        if (BQ == 2) *reinterpret_cast<float4*>(B + (b_kr + NT / 32) * BN + 4 * b_nv) = breg1;
    };

    f32x16 accM, accY[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        accM[r] = 0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o) accY[o][r] = 0.f;
    }

    areg = ld4(Ac);
    breg0 = ld4(Bc);
    breg1 = ld4(Bc + b_half);
    store_tile(0);
    __syncthreads();
    // one K tile from LDS buffer BUF (compile-time, so every ds_read offset is an immediate)
    auto k_tile = [&](auto bufc, bool more, bool last_kt) {
        constexpr int BUF = decltype(bufc)::value;
        if (more) load_next(last_kt);
        const float* A = As + BUF * A_TILE + wm0;
        const float* B = Bs + BUF * B_TILE + wn0 + l31;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float av = A[(kk + h) * BM + (l31 ^ (BK == 32 ? (((kk >> 2) & 7) << 2) : (((kk >> 2) & 3) << 3)))];
            accM = __builtin_amdgcn_mfma_f32_32x32x2f32(av, B[(kk + h) * BN], accM, 0, 0, 0);
        }
        if (more) store_tile(BUF ^ 1);
        __syncthreads();
    };
    for (int xi = 0; xi < 16; ++xi) {
        for (int kt = 0; kt < KT; kt += 2) {   // KT is even (host checks K % 32 == 0)
            k_tile(std::integral_constant<int, 0>{}, true, false);
            const bool last = kt + 2 == KT;
            k_tile(std::integral_constant<int, 1>{}, !(last && xi == 15), last);
        }
        // M_xi complete: fold it into the four outputs, all four products (wino_gemm_g_kernel skips the zero ones)
        const float4 c = wino_out_coeffs<16>(xi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float m = accM[r];
            accY[0][r] += c.x * m; accY[1][r] += c.y * m;
            accY[2][r] += c.z * m; accY[3][r] += c.w * m;
            accM[r] = 0.f;
        }
    }

    // ---- epilogue: D[i][j], i = (r&3) + 8*(r>>2) + 4*h (tile), j = l31 (column)
    const int pa = a.so == 2 ? (phase >> 1) : 0, pb = a.so == 2 ? (phase & 1) : 0;
    const int col = n0 + wn0 + l31;
    const float2 st = wino_store_generic<true>(a, a.y, accY, 0.f, m0 + wm0 + 4 * h, col, pa, pb);
    if (a.stats) wino_store_stats(a, phase, tm, wave & 1, h, col, st.x, st.y);
}

// ---------------------------------------------------------------------------
// The same 16 GEMMs + output transform with LDS-direct loads (buffer_load_dwordx4 ... lds; igemm_nng_kernel in gemm.hip has
// the layouts and the reasoning): 8 waves, wave tile 32 x 32.  A = 64 rows of V (a tile's BK consecutive k = 8 or 4 quads,
// row-major, quad index XOR-ed with swz(row) so that the ds_read_b128 fragment reads are conflict-free), B = BK rows of U
// ([k][n], ds_read_b32 fragments).  A wave instruction fills 1 KB: BK 32 -> every wave brings 8 rows of V and 2 x 2 rows
// of U per K tile; BK 16 -> waves 0..3 bring 16 rows of V each, every wave 2 rows of U.  Rows past the last tile are
// clamped to it (their results are never stored), as in wino_gemm_kernel.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wino_glds16(__amdgpu_buffer_rsrc_t r, float* lds, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)   // device pass only: the host pass would drop the kernel's launch stub (see gemm.hip)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
#endif
}

template <int BK, int NPOS = 16>
__global__ __launch_bounds__(512, 4) void wino_gemm_g_kernel(WinoArgs a) {
    constexpr int BM = 64, BN = 128;
    constexpr int KV = BK / 4, RPW = 64 / KV, G2 = KV / 2;
    constexpr int A_TILE = BK * BM, B_TILE = BK * BN;
    constexpr int AW = BM / RPW;          // waves that bring A rows (8 at BK 32, 4 at BK 16)
    constexpr int BQ = BK / 16;           // B instructions per wave per K tile (16 rows per pass of the 8 waves)
    __shared__ __attribute__((aligned(16))) float As0[A_TILE];
    __shared__ __attribute__((aligned(16))) float As1[A_TILE];
    __shared__ __attribute__((aligned(16))) float Bs0[B_TILE];
    __shared__ __attribute__((aligned(16))) float Bs1[B_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave & 1) * 32, wn0 = (wave >> 1) * 32;
    const WinoPlace pl = wino_place(a.xcd, a.Nc / BN);
    const int tm = pl.tm;
    int phase = pl.phase;
    const int m0 = tm * BM, n0 = pl.tn * BN;
    const int Kext = a.kz ? a.kz : a.K;                           // K rows this workgroup walks, from row koff
    const int koff = a.kz ? phase * a.kz : 0;
    float* const yout = a.y + (a.kz ? (long)phase * a.T * 4 * a.Nc : 0L);
    if (a.kz) phase = 0;
    const int KT = CG_PROBE_HALF(4, Kext / BK);

    // ---- staging: lane -> (row, LDS quad position) of A, (k row, column quad) of B
    const int a_row_l = (wave % AW) * RPW + lane / KV;            // row of the tile block this lane brings (waves >= AW: unused)
    const int a_pos = lane % KV;
    const int a_sw = KV == 8 ? ((a_row_l >> 1) & 7) : ((a_row_l >> 2) & 3);
    const int a_row = min(m0 + a_row_l, a.T - 1);
    const unsigned a_voff = (unsigned)(a_row * a.K + 4 * (a_pos ^ a_sw)) * 4u;
    const int b_kr = wave * 2 + (lane >> 5);                      // + 16 q
    const unsigned b_voff = (unsigned)(b_kr * a.Nc + n0 + 4 * (lane & 31)) * 4u;
    const float* Up = a.U + (long)phase * NPOS * a.K * a.Nc;
    __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)Up, 0, 0x7fffffff, 0x00020000);
    const long a_plane = (long)a.T * a.K;                         // V stride between xi (one plane < 2 GB: host check)
    const float* Vp = a.V + (a.vpp ? (long)phase * NPOS * a_plane : 0L);

    // the next tile to request: (xi, k0), advanced by every dma_tile
    int nxi = 0, nk0 = 0;
    auto dma_tile = [&](auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        float* A = buf ? As1 : As0;
        float* B = buf ? Bs1 : Bs0;
        if (AW == 8 || wave < AW) {
            __amdgpu_buffer_rsrc_t rsv = __builtin_amdgcn_make_buffer_rsrc((void*)(Vp + nxi * a_plane), 0, 0x7fffffff, 0x00020000);
            wino_glds16(rsv, A + (wave % AW) * RPW * BK, a_voff, (koff + nk0) * 4);
        }
        const int sb = (nxi * a.K + koff + nk0) * a.Nc * 4;
#pragma unroll
        for (int q = 0; q < BQ; ++q) wino_glds16(rsu, B + (16 * q + wave * 2) * BN, b_voff + (unsigned)(16 * q * a.Nc) * 4u, sb);
        nk0 += BK;
        if (nk0 >= Kext) { nk0 = 0; ++nxi; }
    };

    f32x16 accM, accY[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        accM[r] = 0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o) accY[o][r] = 0.f;
    }

    dma_tile(std::integral_constant<int, 0>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int f_sw = KV == 8 ? ((l31 >> 1) & 7) : ((l31 >> 2) & 3);
    int qa_rd[G2];
#pragma unroll
    for (int gq = 0; gq < G2; ++gq) qa_rd[gq] = (wm0 + l31) * KV + ((2 * gq + h) ^ f_sw);
    const int qb_rd = 4 * h * BN + wn0 + l31;

    auto k_tile = [&](auto bufc, bool more) {
        constexpr int BUF = decltype(bufc)::value;
        if (more) dma_tile(std::integral_constant<int, BUF ^ 1>{});
        const float4* A4 = reinterpret_cast<const float4*>(BUF ? As1 : As0);
        const float* B = (BUF ? Bs1 : Bs0) + qb_rd;
#pragma unroll
        for (int gq = 0; gq < G2; ++gq) {
            const float4 af = A4[qa_rd[gq]];
#pragma unroll
            for (int sidx = 0; sidx < 4; ++sidx)
                accM = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(af, sidx), B[(8 * gq + sidx) * BN], accM, 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    for (int xi = 0; xi < NPOS; ++xi) {
        for (int kt = 0; kt < KT; kt += 2) {   // KT is even (host checks K % (2 BK) == 0)
            k_tile(std::integral_constant<int, 0>{}, true);
            k_tile(std::integral_constant<int, 1>{}, !(kt + 2 == KT && xi == NPOS - 1));
        }
        // M_xi complete: fold it into the four outputs.  The coefficients are 0 / +-1 and wave-uniform (xi is): a zero term is skipped by a
        // scalar branch - 36 of the 64 products of F(2x2,3x3) (16 of 36 for F(2x2,2x2)) are non-zero, and fp32 MFMA time is VALU time
        // (round 5)
        const float4 c = wino_out_coeffs<NPOS>(xi);
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (f4c(c, o) != 0.f) {
#pragma unroll
                for (int r = 0; r < 16; ++r) accY[o][r] += f4c(c, o) * accM[r];
            }
#pragma unroll
        for (int r = 0; r < 16; ++r) accM[r] = 0.f;
    }

    // ---- epilogue: D[i][j], i = (r&3) + 8*(r>>2) + 4*h (tile), j = l31 (column)
    const int pa = a.so == 2 ? (phase >> 1) : 0, pb = a.so == 2 ? (phase & 1) : 0;
    float st1 = 0.f, st2 = 0.f;
    const int col = n0 + wn0 + l31;
    const float bcol = a.bias ? a.bias[col] : 0.f;
    if (a.lg_tw >= 0) {
        // lean path (round 5): power-of-two tile grids and an output below 2 GB - the tile decode is shifts and masks, the pixel's byte
        // offset one 32-bit value per accumulator row, the four outputs of a tile sit at wave-uniform distances (an SGPR offset of the
        // buffer store), and a row past the last tile stores to the out-of-range offset.  The generic store (two integer divisions
        // per row, a 64-bit address per value) was ~1.5 VALU per MFMA of the whole launch.
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)yout, 0, 0x7fffffff, 0x00020000);
        const int colb = col * 4;
        const int rowp = a.Wo * a.Nc * 4;                      // bytes per output row of pixels
        int soffs[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) soffs[o] = ((o >> 1) * a.so) * rowp + ((o & 1) * a.so) * a.Nc * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int tj = m & (a.tW - 1), ti = (m >> a.lg_tw) & (a.tH - 1), n = m >> (a.lg_tw + a.lg_th);
            const int oy = 2 * ti * a.so + pa, ox = 2 * tj * a.so + pb;
            const unsigned vo = m < a.T ? (unsigned)(((n * a.Ho + oy) * a.Wo + ox) * a.Nc * 4 + colb) : 0x80000000u;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float v = accY[o][r] + bcol;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ry, (int)vo, soffs[o], 0);
                if (a.stats && m < a.T) { st1 += v; st2 += v * v; }
            }
        }
    } else {
        const float2 st = wino_store_generic<false>(a, yout, accY, bcol, m0 + wm0 + 4 * h, col, pa, pb);
        st1 = st.x; st2 = st.y;
    }
    if (a.stats) wino_store_stats(a, phase, tm, wave & 1, h, col, st1, st2);
}

// ---------------------------------------------------------------------------
// The data gradient's 16 GEMMs with the input transform fused in: V is never written.  The unfused pair writes V = 16 T 4Cout floats (268 MB
// on G's 256 -> 128 layer at batch 128) and reads it straight back; nothing else ever reads it.  Here the A operand is formed from dy:
//   workgroup = an 8 x 8 block of tiles of one image (64 GEMM rows) x 64 columns of dx_lo.  K = 4 Cout walks the four phase sub-lattices of
//               dy side by side in steps of 32 planes: the block's 18 x 18 pixel patch of the phase lattice (zero outside the image, the
//               border rule of wino_input_transform_kernel<1>) x 32 planes = one full 128-byte line per pixel goes to LDS by LDS-direct
//               loads, double buffered (2 x 41 KB), and U [16 positions][8 k][64 columns] in sub-steps of 8 k (2 x 32 KB).
//   wave      = ONE row xy of the 4 x 4 positions x one half (32 tiles) of the block, all 64 columns (the structure of wino3.hip): per 8 k
//               eight ds_read_b128 bring rows I1, I2 of B^T's row xy, e = d[I1] -+ d[I2] is shared by the row's four positions,
//               v[nu] = e[J1] -+ e[J2] in wino_input_transform_kernel's operation order (a V element has the bits it has there), and
//               32 v_mfma_f32_32x32x2_f32 (4 positions x 2 column tiles x 4 k pairs) follow on eight accumulators that live through all of
//               K: 32 VALU per 32 MFMAs.  Every product is added in wino_gemm_g_kernel's order, in the K loop and in the output
//               transform (the four rows' waves hand the running sums on through LDS): dx_lo has the unfused pair's bits.
//   LDS image : a patch row holds its even pixel columns first, then the odd ones, 8 plane quads per pixel XORed with
//               ((px >> 2) & 3) * 2 + ((py >> 1) & 1); with the lanes -> tiles permutation of tile_of_row a 16-lane group of
//               ds_read_b128 (two tile rows x eight tile columns, one plane quad) touches 16 distinct 16-byte slots.  The swizzle is
//               applied to the SOURCE address of the LDS-direct loads, the LDS side of one wave instruction is 1 KB of consecutive slots.
// grid = N * ceil(tH/8) * ceil(tW/8) * Nc/64 workgroups of 512 threads, one per CU (150 KB of LDS, 2 waves per SIMD).
// ---------------------------------------------------------------------------
struct WinoFusedArgs {
    const float* dy;     // [N][2 Hl][2 Wl][Cs], Hl = 2 tH, Wl = 2 tW
    const float* U;      // [16][K][Nc], K = 4 Cs
    float* y;            // dx_lo [N][Hl][Wl][Nc]
    int N, tH, tW, Cs, K, Nc;
    int bH, bW;          // 8 x 8 tile blocks per image
    int xcd;             // the column blocks of one tile block on ONE XCD (they share the patch), see wino_gemm_kernel
};
constexpr int kFusedPatchSlots = 18 * 18 * 8;                       // 16-byte slots of a patch: pixels x plane quads
constexpr int kFusedPatchInstr = (kFusedPatchSlots + 63) / 64;      // wave instructions of 64 slots (the last one half empty: zeros)
constexpr int kFusedPatchFloats = kFusedPatchInstr * 64 * 4;
constexpr int kFusedUFloats = 16 * 8 * 64;

__device__ __forceinline__ int fused_pidx(int px) { return (px >> 1) + 9 * (px & 1); }
__device__ __forceinline__ int fused_swz(int py, int px) { return (((px >> 2) & 3) << 1) | ((py >> 1) & 1); }

__global__ __launch_bounds__(512, 2) void wino_dgrad_fused_kernel(WinoFusedArgs a) {
    // four arrays, not one: the compiler must see that an LDS-direct load into one buffer does not feed the reads of the other
    __shared__ __attribute__((aligned(16))) float P0[kFusedPatchFloats];
    __shared__ __attribute__((aligned(16))) float P1[kFusedPatchFloats];
    __shared__ __attribute__((aligned(16))) float U0[kFusedUFloats];
    __shared__ __attribute__((aligned(16))) float U1[kFusedUFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int xy = wave & 3, mh = wave >> 2;
    const int Hl = 2 * a.tH, Wl = 2 * a.tW;
    const int ncb = a.Nc >> 6, nblk = a.N * a.bH * a.bW;
    int cb = blockIdx.x % ncb, blk = blockIdx.x / ncb;
    if (a.xcd && (nblk & 7) == 0) {
        const int slot = blockIdx.x >> 3;
        cb = slot % ncb;
        blk = (slot / ncb) * 8 + (blockIdx.x & 7);
    }
    const int bx = blk % a.bW, by = (blk / a.bW) % a.bH, n = blk / (a.bW * a.bH);
    const int ty0 = by * 8, tx0 = bx * 8, n0 = cb * 64;

    // ---- staging.  dy: one buffer per image (host: below 2 GB); the phase and the plane offset of a K step are the SGPR offset, a lane's
    // pixel and plane quad its VGPR offset, fixed for the whole launch; a pixel outside the image is an out-of-range offset (-> 0)
    const unsigned img_bytes = (unsigned)(4 * Hl * Wl * a.Cs) * 4u;
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dy + (long)n * 4 * Hl * Wl * a.Cs), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)a.U, 0, 0x7fffffff, 0x00020000);
    constexpr int PJ = (kFusedPatchInstr + 7) / 8;     // patch instructions per wave: instruction wave + 8 jj
    unsigned pvoff[PJ];
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj) {
        const int slot = (wave + 8 * jj) * 64 + lane;
        const int pi = slot >> 3, py = pi / 18, pxi = pi - py * 18;
        const int px = pxi < 9 ? 2 * pxi : 2 * (pxi - 9) + 1;
        const int q = (slot & 7) ^ fused_swz(py, px);
        const int iy = 2 * ty0 - 1 + py, ix = 2 * tx0 - 1 + px;
        const bool in = slot < kFusedPatchSlots && iy >= 0 && iy < Hl && ix >= 0 && ix < Wl;
        pvoff[jj] = in ? (unsigned)(((2 * iy * 2 * Wl + 2 * ix) * a.Cs + 4 * q) * 4) : 0x80000000u;
    }
    unsigned uvoff[4];      // U: wave instruction wave * 4 + i = (position, k half), lanes = 4 k rows x 16 column quads
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = wave * 4 + i, pos = idx >> 1, kh = idx & 1;
        uvoff[i] = (unsigned)(((pos * a.K + kh * 4 + (lane >> 4)) * a.Nc + n0 + 4 * (lane & 15)) * 4);
    }
    // part PART (0..3) of the patch of K step kp into buffer PB: instructions jj = 0, 1 | 2, 3 | 4 | 5 of this wave
    auto dma_patch = [&](auto pbc, auto partc, int kp) {
        constexpr int PB = decltype(pbc)::value, PART = decltype(partc)::value;
        constexpr int J0 = PART == 0 ? 0 : (PART == 1 ? 2 : (PART == 2 ? 4 : 5)), J1 = PART == 0 ? 2 : (PART == 1 ? 4 : (PART == 2 ? 5 : 6));
        const int k0 = kp * 32, p = k0 / a.Cs, cs0 = k0 - p * a.Cs;
        const int soff = (((p >> 1) * 2 * Wl + (p & 1)) * a.Cs + cs0) * 4;
#pragma unroll
        for (int jj = J0; jj < J1 && jj < PJ; ++jj)
            if (wave + 8 * jj < kFusedPatchInstr) wino_glds16(rsd, (PB ? P1 : P0) + (wave + 8 * jj) * 256, pvoff[jj], soff);
    };
    auto dma_u = [&](auto ubc, int k) {       // the 8 K rows from k on, all 16 positions
        constexpr int UB = decltype(ubc)::value;
        const int soff = k * a.Nc * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) wino_glds16(rsu, (UB ? U1 : U0) + (wave * 4 + i) * 256, uvoff[i], soff);
    };

    // ---- fragments: the wave's row xy of B^T takes patch rows I1 -+ I2 (0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3)
    const int I1 = xy == 0 ? 0 : (xy == 2 ? 2 : 1), I2 = xy == 0 ? 2 : (xy == 1 ? 2 : (xy == 2 ? 1 : 3));
    const int tl = cg::tile_of_row(j), tyl = (tl >> 3) + 4 * mh, txl = tl & 7;
    int pa_rd[2][4];        // byte address in a patch buffer of (row I1 / I2, column c), plane quad h; K sub-step s: ^ (s << 5)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int py = 2 * tyl + (rr ? I2 : I1), px = 2 * txl + c;
            pa_rd[rr][c] = ((py * 18 + fused_pidx(px)) * 8 + (h ^ fused_swz(py, px))) * 16;
        }
    const float sgn = xy == 1 ? 1.f : -1.f;      // e = d[I1] + sgn * d[I2]: the product is exact, the sum has the bits of the plain + / -
    const int ub_rd = xy * 4 * 512 + h * 4 * 64 + j;     // U fragment: + nu * 512 + comp * 64 + ni * 32

    f32x16 acc[4][2];
#pragma unroll
    for (int nu = 0; nu < 4; ++nu)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nu][ni][r] = 0.f;

    using I0c = std::integral_constant<int, 0>;
    using I1c = std::integral_constant<int, 1>;
    using I2c = std::integral_constant<int, 2>;
    using I3c = std::integral_constant<int, 3>;
    const int KP = CG_PROBE_HALF(4, a.K / 32);      // K steps of 32 planes, even (host: K % 512 == 0)
    dma_patch(I0c{}, I0c{}, 0); dma_patch(I0c{}, I1c{}, 0); dma_patch(I0c{}, I2c{}, 0); dma_patch(I0c{}, I3c{}, 0);
    dma_u(I0c{}, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // K sub-step S (8 planes) of K step kp from patch buffer PB and U buffer S & 1; requests the next sub-step's U and a part of the next patch
    auto sub_step = [&](auto pbc, auto sc, int kp) {
        constexpr int PB = decltype(pbc)::value, S = decltype(sc)::value;
        const bool more_p = kp + 1 < KP;
        if (more_p) dma_patch(std::integral_constant<int, PB ^ 1>{}, sc, kp + 1);
        if (S < 3 || more_p) dma_u(std::integral_constant<int, (S & 1) ^ 1>{}, kp * 32 + 8 * S + 8);
        const char* P = reinterpret_cast<const char*>(PB ? P1 : P0);
        const float* B = ((S & 1) ? U1 : U0) + ub_rd;
        // MFMA (S, comp) contracts planes 8 S + comp (lane half 0) and 8 S + 4 + comp (lane half 1) and rotates over the eight accumulators.
        // Software-pipelined by hand: the U fragments and the A values of k pair comp + 1 are requested / formed before the MFMAs of k pair
        // comp are issued (left to itself the compiler reads every U pair right in front of its two MFMAs: same time alone, but the step
        // gained nothing - profiles/wino_dgrad_fused.txt)
        float4 d1[4], d2[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            d1[c] = *reinterpret_cast<const float4*>(P + (pa_rd[0][c] ^ (S << 5)));
            d2[c] = *reinterpret_cast<const float4*>(P + (pa_rd[1][c] ^ (S << 5)));
        }
        auto frag = [&](int comp, float (&o)[4]) {     // e = d[I1] -+ d[I2] per patch column, then B's columns: e0 - e2, e1 + e2, e2 - e1, e1 - e3
            float e[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) e[c] = __builtin_fmaf(sgn, f4c(d2[c], comp), f4c(d1[c], comp));
            o[0] = e[0] - e[2]; o[1] = e[1] + e[2]; o[2] = e[2] - e[1]; o[3] = e[1] - e[3];
        };
        float b[2][8], v[2][4];      // [k pair & 1][position nu * 2 + column tile ni], [k pair & 1][nu]
#pragma unroll
        for (int i = 0; i < 8; ++i) b[0][i] = B[(i >> 1) * 512 + (i & 1) * 32];
        frag(0, v[0]);
#pragma unroll
        for (int comp = 0; comp < 4; ++comp) {
            if (comp < 3) {
#pragma unroll
                for (int i = 0; i < 8; ++i) b[(comp + 1) & 1][i] = B[(i >> 1) * 512 + (comp + 1) * 64 + (i & 1) * 32];
                frag(comp + 1, v[(comp + 1) & 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i >> 1][i & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[comp & 1][i >> 1], b[comp & 1][i], acc[i >> 1][i & 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    for (int kp = 0; kp < KP; kp += 2) {
        sub_step(I0c{}, I0c{}, kp); sub_step(I0c{}, I1c{}, kp); sub_step(I0c{}, I2c{}, kp); sub_step(I0c{}, I3c{}, kp);
        sub_step(I1c{}, I0c{}, kp + 1); sub_step(I1c{}, I1c{}, kp + 1); sub_step(I1c{}, I2c{}, kp + 1); sub_step(I1c{}, I3c{}, kp + 1);
    }

    // ---- output transform, with the bits of wino_gemm_g_kernel: there one wave walks xi = 0..15 and adds every finished M_xi to the outputs
    // it feeds, one after the other (Y_o = ((0 + c M_0) + c M_1) + ...; A^T = [1 1 1 0; 0 1 -1 -1] on both axes).  Here the rows of the positions
    // sit in four waves, so the running sums pass from the wave of row 0 to that of row 3 through LDS (the patch buffer of the wave's tile
    // half, dead after the loop's last barrier): [output o][column tile ni][1024 floats].  Row xy adds its positions in the order xx = 0..3;
    // outputs 0, 1 (first row of A^T) are complete after row 2, outputs 2, 3 after row 3.  The K loop adds every product in
    // wino_gemm_g_kernel's order as well, so dx_lo is the transform + GEMM pair's bit for bit.
    static_assert(kFusedPatchFloats >= 8 * 1024, "the epilogue's exchange fits in a patch buffer");
    const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc((void*)(a.y + (long)n * Hl * Wl * a.Nc), 0, (unsigned)(Hl * Wl * a.Nc) * 4u, 0x00020000);
    const int rowb = 2 * Wl * a.Nc * 4, colb = 2 * a.Nc * 4;       // bytes per tile row / tile column of dx_lo
    float* const X = mh ? P1 : P0;
    // accumulator row r of lane half h is MFMA row (r & 3) + 8 (r >> 2) + 4 h -> tile_of_row(): a compile-time tile per (r, h)
    auto store_out = [&](int o, int ni, const f32x16& Y) {
        const int lane_base = (((2 * ty0 + (o >> 1)) * Wl + 2 * tx0 + (o & 1)) * a.Nc + n0 + ni * 32 + j) * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row0 = (r & 3) + 8 * (r >> 2);
            const int t = h ? cg::tile_of_row_c(row0 + 4) : cg::tile_of_row_c(row0);
            const int ty = (t >> 3) + 4 * mh, tx = t & 7;
            const bool in = ty0 + ty < a.tH && tx0 + tx < a.tW;     // a partly filled block: tiles past the image's grid are not stored
            const unsigned vo = in ? (unsigned)(lane_base + ty * rowb + tx * colb) : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(Y[r] + 0.f), rsy, (int)vo, 0, 0);     // + 0.f: the pair's "+ bias" without one
        }
    };
    const float cyr[2] = {xy < 3 ? 1.f : 0.f, xy == 0 ? 0.f : (xy == 1 ? 1.f : -1.f)};     // column xy of A^T
    // this wave's row added to output o of column tile ni: the running sum comes from LDS unless the row is the output's first
    auto add_row = [&](int o, int ni, f32x16& Y) {
        const bool first = (o >> 1) == 0 ? xy == 0 : xy == 1;
        float* Xo = X + (o * 2 + ni) * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[r] = first ? 0.f : Xo[r * 64 + lane];
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
            const float cx = (o & 1) == 0 ? (xx < 3 ? 1.f : 0.f) : (xx == 0 ? 0.f : (xx == 1 ? 1.f : -1.f));
            const float c = cyr[o >> 1] * cx;
            if (c != 0.f) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[r] += c * acc[xx][ni][r];
            }
        }
    };
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        if (xy == row) {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (cyr[o >> 1] == 0.f) continue;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    f32x16 Y;
                    add_row(o, ni, Y);
                    if (row == 3) store_out(o, ni, Y);      // outputs 2, 3 are complete
                    else {
                        float* Xo = X + (o * 2 + ni) * 1024;
#pragma unroll
                        for (int r = 0; r < 16; ++r) Xo[r * 64 + lane] = Y[r];
                    }
                }
            }
        } else if (row == 3 && xy < 2) {     // meanwhile the waves of rows 0 and 1 store the complete outputs 0 and 1
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                f32x16 Y;
                const float* Xo = X + (xy * 2 + ni) * 1024;
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[r] = Xo[r * 64 + lane];
                if (xy == 0) store_out(0, ni, Y); else store_out(1, ni, Y);
            }
        }
        if (row < 3) __syncthreads();
    }
}

__device__ __host__ __forceinline__ int wino_phase_map(int a, int d) { return ((a + d - 2) >> 1) - ((a - 2) >> 1); }

// gw[co][ci][5][5] += scale * sum_p (G^T dU_p G)[map_p(dy,dx)];  dUt layout [xi][p*Cout+co][ci].  One thread per (co, ci).
__global__ __launch_bounds__(256) void wino_wgrad_finish_kernel(const float* __restrict__ dUt, float* __restrict__ gw, int Cout,
                                                                int Cin, float scale) {
    const long total = (long)Cout * Cin;
    const long xs = 4L * Cout * Cin;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += gridDim.x * 256L) {
        const int ci = (int)(idx % Cin);
        const int co = (int)(idx / Cin);
        float acc[25];
#pragma unroll
        for (int t = 0; t < 25; ++t) acc[t] = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float u[4][4];
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) u[xi >> 2][xi & 3] = dUt[xi * xs + ((long)p * Cout + co) * Cin + ci];
            float t[3][4];  // G^T u, G^T = [1 .5 .5 0; 0 .5 -.5 0; 0 .5 .5 1]
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                t[0][c] = u[0][c] + 0.5f * (u[1][c] + u[2][c]);
                t[1][c] = 0.5f * (u[1][c] - u[2][c]);
                t[2][c] = 0.5f * (u[1][c] + u[2][c]) + u[3][c];
            }
            float g[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                g[r][0] = t[r][0] + 0.5f * (t[r][1] + t[r][2]);
                g[r][1] = 0.5f * (t[r][1] - t[r][2]);
                g[r][2] = 0.5f * (t[r][1] + t[r][2]) + t[r][3];
            }
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) acc[dy * 5 + dx] += g[wino_phase_map(p >> 1, dy)][wino_phase_map(p & 1, dx)];
        }
        float* dst = gw + idx * 25;
#pragma unroll
        for (int t = 0; t < 25; ++t) dst[t] += scale * acc[t];
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
bool wino_dims_ok(int N, int Hp, int Wp, int Cin, int Cout) {
    return N > 0 && Hp > 0 && Wp > 0 && (Hp & 1) == 0 && (Wp & 1) == 0 && Cin > 0 && Cout > 0 && Cin % 128 == 0 &&
           Cout % 128 == 0 /* K % 32, Nc % 128 for both GEMM geometries */ && (long)N * Hp * Wp * std::max(Cin, 4 * Cout) * 4L < (1L << 40);
}

// May wino_gemm_g_kernel take T tiles x K rows x Nc columns: LDS-direct loads are on (CG_WINO_GLDS), and one xi plane of V and the planes
// of U stay below the 2 GB a buffer offset reaches
bool glds_ok(long T, int K, int Nc) {
    return cg::opt(cg::OPT_WINO_GLDS) != 0 && T * K * 4L < 0x7fffffffL && 16L * K * Nc * 4L < 0x7fffffffL;
}

// The GEMMs + output transform on an already transformed input: npos = 16 (F(2x2,3x3)) or 9 (F(2x2,2x2)) positions.
// dgrad == 0: v [npos][T][Cin] (npos == 9: per phase), u = u_fwd, y [N][2Hp][2Wp][Cout];  dgrad == 1: v [npos][T][4*Cout], u = u_bwd,
// y [N][Hp][Wp][Cin], or with kslices > 1 that many partial results T*4*Cin floats apart (K slices over blockIdx.z).
int wino_gemm_launch(void* stream, const float* v, const float* u, const float* bias, float* y, int N, int Hp, int Wp,
                     int Cin, int Cout, int dgrad, float* stats, int npos, int kslices) {
    CG_REQUIRE(v && u && y, "cg_conv2d_ups2_wino_gemm: null pointer");
    CG_REQUIRE(wino_dims_ok(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino_gemm: unsupported dimensions");
    const int T = N * (Hp / 2) * (Wp / 2);
    WinoArgs a;
    a.V = v; a.U = u; a.bias = bias; a.y = y; a.T = T; a.tH = Hp / 2; a.tW = Wp / 2; a.stats = stats;
    a.xcd = (int)cg::opt(cg::OPT_XCD_SWIZZLE);
    a.vpp = npos == 9 && !dgrad ? 1 : 0;
    a.kz = 0;
    a.lg_tw = a.lg_th = -1;
    CG_REQUIRE(!stats || !dgrad, "wino_gemm: statistics only on the forward launch");
    if (dgrad) { a.K = 4 * Cout; a.Nc = Cin; a.so = 1; a.Ho = Hp; a.Wo = Wp; }
    else { a.K = Cin; a.Nc = Cout; a.so = 2; a.Ho = 2 * Hp; a.Wo = 2 * Wp; }
    const int bk = (int)cg::opt(cg::OPT_WINO_BK);
    CG_REQUIRE(kslices <= 1 || (dgrad && a.K % kslices == 0 && (a.K / kslices) % 64 == 0), "wino_gemm: K slices only on the data gradient, in multiples of 64 rows");
    if (kslices > 1) a.kz = a.K / kslices;
    {
        auto lg = [](int v) { int l = 0; while ((1 << l) < v) ++l; return (1 << l) == v ? l : -1; };
        const long ybytes = (long)N * a.Ho * a.Wo * a.Nc * 4L;
        if (lg(a.tW) >= 0 && lg(a.tH) >= 0 && ybytes < 0x7fffffffL) { a.lg_tw = lg(a.tW); a.lg_th = lg(a.tH); }
    }
    const dim3 grid(cg::cdiv(T, 64) * (a.Nc / 128), 1, dgrad ? (kslices > 1 ? kslices : 1) : 4);
    // K step 32 (half the barriers per MFMA) pays when the launch is at most ~one workgroup per CU - the data-gradient
    // geometry at batch 128 (0.53 -> 0.41 ms) - and costs 6 % when two workgroups per CU already hide each other's barriers;
    // it needs an even number of K tiles per workgroup
    const bool k32 = (bk == 32 || (bk == 0 && (long)grid.x * grid.z <= cg::kNumCU * 3 / 2)) && (a.kz ? a.kz : a.K) % 64 == 0;
    const bool glds = glds_ok(T, a.K, a.Nc);
    // F(2x2,2x2) has the LDS-direct-load kernel only (cg_conv2d_ups2_wino22_supported asks the same question)
    CG_REQUIRE(npos == 16 || glds, "wino_gemm: the 9-position form needs the LDS-direct-load kernel (CG_WINO_GLDS)");
    CG_REQUIRE(kslices <= 1 || glds, "wino_gemm: K slices need the LDS-direct-load kernel (CG_WINO_GLDS)");
    hipStream_t st = cg::S(stream);
    if (npos == 9) {
        if (k32) hipLaunchKernelGGL((wino_gemm_g_kernel<32, 9>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((wino_gemm_g_kernel<16, 9>), grid, dim3(512), 0, st, a);
    } else if (glds) {
        if (k32) hipLaunchKernelGGL((wino_gemm_g_kernel<32>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((wino_gemm_g_kernel<16>), grid, dim3(512), 0, st, a);
    } else {
        if (k32) hipLaunchKernelGGL((wino_gemm_kernel<32>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((wino_gemm_kernel<16>), grid, dim3(512), 0, st, a);
    }
    CG_LAUNCH_CHECK();
    return 0;
}

// Both *_pack entry points: both operands in one launch (CG_PACK_WIDE) or a launch per operand that is asked for
template <class F>
int wino_pack(const char* who, void* stream, const float* wf_ph, const float* wb_ph, float* u_fwd, float* u_bwd, int Cout, int Cin) {
    CG_REQUIRE((wf_ph && u_fwd) || (wb_ph && u_bwd), "%s: null pointer", who);
    CG_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0, "%s: channel counts must be multiples of 4", who);
    hipStream_t st = cg::S(stream);
    const int nf = cg::ew_grid(4L * Cin * (Cout / 4)), nb = cg::ew_grid(4L * Cout * (Cin / 4));
    if (wf_ph && u_fwd && wb_ph && u_bwd && cg::opt(cg::OPT_PACK_WIDE) != 0) {
        hipLaunchKernelGGL(wino_filter_transform_both_kernel<F>, dim3(nf + nb), dim3(256), 0, st, wf_ph, u_fwd, wb_ph, u_bwd, Cin, Cout, nf);
        CG_LAUNCH_CHECK();
        return 0;
    }
    if (wf_ph && u_fwd) {
        hipLaunchKernelGGL((wino_filter_transform_kernel<F, false>), dim3(nf), dim3(256), 0, st, wf_ph, u_fwd, Cin, Cout);
        CG_LAUNCH_CHECK();
    }
    if (wb_ph && u_bwd) {
        hipLaunchKernelGGL((wino_filter_transform_kernel<F, true>), dim3(nb), dim3(256), 0, st, wb_ph, u_bwd, Cout, Cin);
        CG_LAUNCH_CHECK();
    }
    return 0;
}

// The unfused data gradient of both families: dy's transform into v_dy, then the GEMMs - in one launch (sl == 1), or with the K rows (the
// four phases' channels) in sl = 2 or 4 slices over blockIdx.z, each writing a partial dx_lo to part, added in a fixed order.
int wino_dgrad_pair(void* stream, const float* dy, const float* u_bwd, float* dx_lo, float* v_dy, float* part, int N, int Hp, int Wp,
                    int Cin, int Cout, int npos, int sl) {
    hipStream_t st = cg::S(stream);
    const int T = N * (Hp / 2) * (Wp / 2);
    const dim3 tgrid(cg::ew_grid((long)T * Cout));
    if (npos == 16) hipLaunchKernelGGL(wino_input_transform_kernel<1>, tgrid, dim3(256), 0, st, dy, v_dy, N, Hp, Wp, 4 * Cout, Cout);
    else hipLaunchKernelGGL(wino22_dy_input_transform_kernel, tgrid, dim3(256), 0, st, dy, v_dy, N, Hp, Wp, Cout);
    CG_LAUNCH_CHECK();
    if (sl <= 1) return wino_gemm_launch(stream, v_dy, u_bwd, nullptr, dx_lo, N, Hp, Wp, Cin, Cout, 1, nullptr, npos, 1);
    if (wino_gemm_launch(stream, v_dy, u_bwd, nullptr, part, N, Hp, Wp, Cin, Cout, 1, nullptr, npos, sl)) return 1;
    const long n = (long)T * 4 * Cin;
    if (sl == 4) hipLaunchKernelGGL(wino22_sum_kernel<4>, dim3(cg::ew_grid(n / 4)), dim3(256), 0, st, part, dx_lo, n / 4, n);
    else hipLaunchKernelGGL(wino22_sum_kernel<2>, dim3(cg::ew_grid(n / 4)), dim3(256), 0, st, part, dx_lo, n / 4, n);
    CG_LAUNCH_CHECK();
    return 0;
}

// K slices of the F(2x2,2x2) data gradient, 1 (unsplit) or 4.  The launch has T/64 x Cin/128 workgroups - 128 on G's 512 -> 256 layer at
// batch 128, half the chip.  Below ~one workgroup per CU the four phases (K slices of Cout rows) go to blockIdx.z.
int wino22_dgrad_slices(int N, int Hp, int Wp, int Cin, int Cout) {
    if (Cout % 64 != 0) return 1;
    return (long)cg::cdiv(N * (Hp / 2) * (Wp / 2), 64) * (Cin / 128) < cg::kNumCU ? 4 : 1;
}

// K slices of the F(2x2,3x3) data gradient, 1, 2 or 4: at one workgroup per CU or more the unsplit launch stays (G32up-c's layer at batch
// 128: 256 workgroups, splitting measured +0.5 % on the step), below that 2 or 4 slices (G32up's 128 -> 256 layer at batch 256: 64
// workgroups -> 4 slices, config #3 9.52 -> 9.25 ms)
int wino_dgrad_slices(int N, int Hp, int Wp, int Cin, int Cout) {
    const long T = (long)N * (Hp / 2) * (Wp / 2);
    if (!glds_ok(T, 4 * Cout, Cin) || !wino_dims_ok(N, Hp, Wp, Cin, Cout)) return 1;
    const long wgs = (long)cg::cdiv((int)T, 64) * (Cin / 128);
    int sl = wgs >= cg::kNumCU ? 1 : (wgs * 2 >= cg::kNumCU ? 2 : 4);
    while (sl > 1 && (4 * Cout / sl) % 64 != 0) sl >>= 1;
    return sl;
}

// With CG_WINO_DGRAD_FUSE != 0 the input transform is fused into the GEMMs (wino_dgrad_fused_kernel) and v_dy is left untouched:
// 1 (default) where the fused kernel supports the shape and wins - whole 8 x 8 tile blocks and at least one workgroup per CU -, 2 wherever
// it supports the shape (tests), 0 = the transform + wino_gemm_g_kernel pair everywhere.  Returns true = takes the fused path.
bool wino_dgrad_fused_takes(const float* dy, const float* u_bwd, const float* dx_lo, int N, int Hp, int Wp, int Cin, int Cout) {
    const long mode = cg::opt(cg::OPT_WINO_DGRAD_FUSE);
    if (mode == 0) return false;
    const int tH = Hp / 2, tW = Wp / 2, bH = cg::cdiv(tH, 8), bW = cg::cdiv(tW, 8);
    const long wgs = (long)N * bH * bW * (Cin / 64);
    // one image of dy / of dx_lo and all of U within a buffer descriptor's 2 GB; K = 4 Cout in an even number of 32-plane steps
    const bool fits = 4L * Hp * Wp * Cout * 4L < 0x7fffffffL && (long)Hp * Wp * Cin * 4L < 0x7fffffffL && 16L * 4L * Cout * Cin * 4L < 0x7fffffffL &&
                      Cout % 32 == 0 && Cin % 64 == 0 && wgs <= 0x7fffffffL &&
                      ((uintptr_t)dy % 16) == 0 && ((uintptr_t)u_bwd % 16) == 0 && ((uintptr_t)dx_lo % 4) == 0;
    if (!fits) return false;
    return mode == 2 || (tH % 8 == 0 && tW % 8 == 0 && wgs >= cg::kNumCU);
}

size_t wino_align(size_t b) { return (b + 255) / 256 * 256; }
// gradBias scratch of the weight gradient's workspace: cg_bias_grad needs Cout doubles; the region keeps the size it had when the dy
// transform left per-workgroup partial sums there, because compiled plans size and lay out their buffers from the byte count below
size_t wino_bias_ws_bytes(int Cout) { return wino_align(std::max(sizeof(double) * Cout, (size_t)cg::kNumCU * 8 * 4 * Cout * sizeof(float))); }

}  // namespace

extern "C" {

// 1 if the Winograd path covers upsample2 -> conv 5x5 (pad 2) at these dimensions
size_t cg_conv2d_ups2_wino_supported(int N, int Hp, int Wp, int Cin, int Cout, int k, int pad) {
    return k == 5 && pad == 2 && wino_dims_ok(N, Hp, Wp, Cin, Cout) ? 1 : 0;
}
size_t cg_conv2d_ups2_wino_v_floats(int N, int Hp, int Wp, int C) {  // C = Cin (forward) or 4*Cout (data gradient)
    return (size_t)16 * ((size_t)N * (Hp / 2) * (Wp / 2)) * C;
}
size_t cg_conv2d_ups2_wino_u_floats(int Cin, int Cout) { return (size_t)4 * 16 * Cin * Cout; }

int cg_conv2d_ups2_wino_pack(void* stream, const float* wf_ph, const float* wb_ph, float* u_fwd, float* u_bwd, int Cout,
                             int Cin) {
    return wino_pack<WinoF23>("cg_conv2d_ups2_wino_pack", stream, wf_ph, wb_ph, u_fwd, u_bwd, Cout, Cin);
}

// The 16 GEMMs + output transform alone, on an already transformed input (what the entry points below launch after
// their input transform; exported so that it can be timed / profiled in isolation).
int cg_conv2d_ups2_wino_gemm(void* stream, const float* v, const float* u, const float* bias, float* y, int N, int Hp, int Wp,
                             int Cin, int Cout, int dgrad) {
    return wino_gemm_launch(stream, v, u, bias, y, N, Hp, Wp, Cin, Cout, dgrad, nullptr, 16, 1);
}

// rows of the [rows][2][Cout] statistics buffer cg_conv2d_ups2_wino_forward_stats fills
size_t cg_conv2d_ups2_wino_stats_rows(int N, int Hp, int Wp, int Cin, int Cout) {
    if (!wino_dims_ok(N, Hp, Wp, Cin, Cout)) return 0;
    return (size_t)4 * cg::cdiv((long)N * (Hp / 2) * (Wp / 2), 64) * 2;
}

// y[N][2Hp][2Wp][Cout] = bias + conv5x5(upsample2(x_lo)); v (cg_conv2d_ups2_wino_v_floats(..., Cin) floats) receives
// the transformed input and is what the weight gradient consumes later.
int cg_conv2d_ups2_wino_forward_stats(void* stream, const float* x_lo, const float* u_fwd, const float* bias, float* y, float* v,
                                      int N, int Hp, int Wp, int Cin, int Cout, float* stats) {
    CG_REQUIRE(x_lo && u_fwd && y && v, "cg_conv2d_ups2_wino_forward: null pointer");
    CG_REQUIRE(wino_dims_ok(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino_forward: unsupported dimensions");
    const int T = N * (Hp / 2) * (Wp / 2);
    hipLaunchKernelGGL(wino_input_transform_kernel<0>, dim3(cg::ew_grid((long)T * (Cin / 4))), dim3(256), 0, cg::S(stream), x_lo, v, N, Hp,
                       Wp, Cin, Cin);
    CG_LAUNCH_CHECK();
    return wino_gemm_launch(stream, v, u_fwd, bias, y, N, Hp, Wp, Cin, Cout, 0, stats, 16, 1);
}

int cg_conv2d_ups2_wino_forward(void* stream, const float* x_lo, const float* u_fwd, const float* bias, float* y, float* v,
                                int N, int Hp, int Wp, int Cin, int Cout) {
    return cg_conv2d_ups2_wino_forward_stats(stream, x_lo, u_fwd, bias, y, v, N, Hp, Wp, Cin, Cout, nullptr);
}

// ---- F(2x2,2x2): upsample2 -> conv 3x3 (pad 1) ----
size_t cg_conv2d_ups2_wino22_supported(int N, int Hp, int Wp, int Cin, int Cout) {
    return wino_dims_ok(N, Hp, Wp, Cin, Cout) && glds_ok((long)N * (Hp / 2) * (Wp / 2), Cin, Cout) ? 1 : 0;
}
// the limits cg_conv2d_ups2_wino22_dgrad applies on top of the forward's (a planner that only asked the forward's
// question would compile the forward and fail in Module:backward for a large batch x Cout)
size_t cg_conv2d_ups2_wino22_dgrad_supported(int N, int Hp, int Wp, int Cin, int Cout) {
    return cg_conv2d_ups2_wino22_supported(N, Hp, Wp, Cin, Cout) && glds_ok((long)N * (Hp / 2) * (Wp / 2), 4 * Cout, Cin) ? 1 : 0;
}
size_t cg_conv2d_ups2_wino22_v_floats(int N, int Hp, int Wp, int Cin) { return (size_t)36 * ((size_t)N * (Hp / 2) * (Wp / 2)) * Cin; }
size_t cg_conv2d_ups2_wino22_u_floats(int Cin, int Cout) { return (size_t)4 * 9 * Cin * Cout; }

int cg_conv2d_ups2_wino22_pack(void* stream, const float* wf_ph, const float* wb_ph, float* u_fwd, float* u_bwd, int Cout, int Cin) {
    return wino_pack<WinoF22>("cg_conv2d_ups2_wino22_pack", stream, wf_ph, wb_ph, u_fwd, u_bwd, Cout, Cin);
}

// y[N][2Hp][2Wp][Cout] = bias + conv3x3(upsample2(x_lo)); v: scratch of cg_conv2d_ups2_wino22_v_floats floats; stats as
// cg_conv2d_ups2_wino_forward_stats (same rows: cg_conv2d_ups2_wino_stats_rows).
int cg_conv2d_ups2_wino22_forward_stats(void* stream, const float* x_lo, const float* u22, const float* bias, float* y, float* v,
                                        int N, int Hp, int Wp, int Cin, int Cout, float* stats) {
    CG_REQUIRE(x_lo && u22 && y && v, "cg_conv2d_ups2_wino22_forward: null pointer");
    CG_REQUIRE(cg_conv2d_ups2_wino22_supported(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino22_forward: unsupported dimensions / options");
    const int T = N * (Hp / 2) * (Wp / 2);
    hipLaunchKernelGGL(wino22_input_transform_kernel, dim3(cg::ew_grid((long)T * (Cin / 4))), dim3(256), 0, cg::S(stream), x_lo, v, N, Hp, Wp, Cin);
    CG_LAUNCH_CHECK();
    return wino_gemm_launch(stream, v, u22, bias, y, N, Hp, Wp, Cin, Cout, 0, stats, 9, 1);
}

size_t cg_conv2d_ups2_wino22_dgrad_v_floats(int N, int Hp, int Wp, int Cin, int Cout) {
    const size_t T = (size_t)N * (Hp / 2) * (Wp / 2);
    const int sl = wino22_dgrad_slices(N, Hp, Wp, Cin, Cout);
    return 36 * T * Cout + (sl > 1 ? (size_t)sl * 4 * T * Cin : 0);
}

// dx_lo[N][Hp][Wp][Cin] = gradient of upsample2 -> conv3x3 w.r.t. the low-res input; v_dy: scratch of cg_conv2d_ups2_wino22_dgrad_v_floats()
// floats (9 planes x T x 4 Cout, + the four partial results when the K slices are split); u_bwd from cg_conv2d_ups2_wino22_pack.
int cg_conv2d_ups2_wino22_dgrad(void* stream, const float* dy, const float* u_bwd, float* dx_lo, float* v_dy, int N, int Hp, int Wp, int Cin,
                                int Cout) {
    CG_REQUIRE(dy && u_bwd && dx_lo && v_dy, "cg_conv2d_ups2_wino22_dgrad: null pointer");
    CG_REQUIRE(cg_conv2d_ups2_wino22_dgrad_supported(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino22_dgrad: unsupported dimensions / options");
    const size_t T = (size_t)N * (Hp / 2) * (Wp / 2);
    return wino_dgrad_pair(stream, dy, u_bwd, dx_lo, v_dy, v_dy + 36 * T * Cout, N, Hp, Wp, Cin, Cout, 9, wino22_dgrad_slices(N, Hp, Wp, Cin, Cout));
}

// dx_lo[N][Hp][Wp][Cin] = gradient w.r.t. the low-res input (the upsampling's 2x2 block sum folded in);
// v_dy: scratch of cg_conv2d_ups2_wino_v_floats(..., 4*Cout) floats, untouched where the fused kernel runs (wino_dgrad_fused_takes).
int cg_conv2d_ups2_wino_dgrad(void* stream, const float* dy, const float* u_bwd, float* dx_lo, float* v_dy, int N, int Hp,
                              int Wp, int Cin, int Cout) {
    CG_REQUIRE(dy && u_bwd && dx_lo && v_dy, "cg_conv2d_ups2_wino_dgrad: null pointer");
    CG_REQUIRE(wino_dims_ok(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino_dgrad: unsupported dimensions");
    if (wino_dgrad_fused_takes(dy, u_bwd, dx_lo, N, Hp, Wp, Cin, Cout)) {
        WinoFusedArgs f;
        f.dy = dy; f.U = u_bwd; f.y = dx_lo; f.N = N; f.tH = Hp / 2; f.tW = Wp / 2; f.Cs = Cout; f.K = 4 * Cout; f.Nc = Cin;
        f.bH = cg::cdiv(f.tH, 8); f.bW = cg::cdiv(f.tW, 8);
        f.xcd = (int)cg::opt(cg::OPT_XCD_SWIZZLE);
        hipLaunchKernelGGL(wino_dgrad_fused_kernel, dim3((unsigned)(N * f.bH * f.bW * (Cin / 64))), dim3(512), 0, cg::S(stream), f);
        CG_LAUNCH_CHECK();
        cg::opt_count(cg::OPT_WINO_DGRAD_FUSE_LAUNCHES);
        return 0;
    }
    return wino_dgrad_pair(stream, dy, u_bwd, dx_lo, v_dy, nullptr, N, Hp, Wp, Cin, Cout, 16, 1);
}

// The same data gradient with its K rows in 2 or 4 slices (wino_dgrad_slices): the unsplit launch has T/64 x Cin/128 workgroups, which
// leaves most of the chip idle where Cin is 128 (G32up's first 5x5 layer).  part: cg_conv2d_ups2_wino_dgrad_part_floats() floats
// (0 = keep the unsplit launch).
size_t cg_conv2d_ups2_wino_dgrad_part_floats(int N, int Hp, int Wp, int Cin, int Cout) {
    const int sl = wino_dgrad_slices(N, Hp, Wp, Cin, Cout);
    return sl > 1 ? (size_t)sl * N * Hp * Wp * Cin : 0;
}
int cg_conv2d_ups2_wino_dgrad_split(void* stream, const float* dy, const float* u_bwd, float* dx_lo, float* v_dy, float* part, int N, int Hp,
                                    int Wp, int Cin, int Cout) {
    const int sl = wino_dgrad_slices(N, Hp, Wp, Cin, Cout);
    if (sl <= 1 || !part) return cg_conv2d_ups2_wino_dgrad(stream, dy, u_bwd, dx_lo, v_dy, N, Hp, Wp, Cin, Cout);
    CG_REQUIRE(dy && u_bwd && dx_lo && v_dy, "cg_conv2d_ups2_wino_dgrad_split: null pointer");
    return wino_dgrad_pair(stream, dy, u_bwd, dx_lo, v_dy, part, N, Hp, Wp, Cin, Cout, 16, sl);
}

size_t cg_conv2d_ups2_wino_wgrad_workspace_bytes(int N, int Hp, int Wp, int Cin, int Cout) {
    if (!wino_dims_ok(N, Hp, Wp, Cin, Cout)) return 0;
    const size_t T = (size_t)N * (Hp / 2) * (Wp / 2);
    return wino_align(16 * T * 4 * Cout * sizeof(float)) + wino_align((size_t)16 * 4 * Cout * Cin * sizeof(float)) + wino_bias_ws_bytes(Cout) +
           cg_conv2d_wgrad_workspace_bytes_strided(16, (int)T, 1, 1, Cin, 4 * Cout, 1, 1, 0, 0, 0);
}

// gw_canonical[Cout][Cin][5][5] += scale * dW, gb += scale * sum dy, from the transformed input v the forward left behind.
int cg_conv2d_ups2_wino_wgrad(void* stream, const float* v, const float* dy, float* gw_canonical, float* gb, int N, int Hp,
                              int Wp, int Cin, int Cout, float scale, void* ws, size_t ws_bytes) {
    CG_REQUIRE(v && dy && gw_canonical, "cg_conv2d_ups2_wino_wgrad: null pointer");
    CG_REQUIRE(wino_dims_ok(N, Hp, Wp, Cin, Cout), "cg_conv2d_ups2_wino_wgrad: unsupported dimensions");
    const size_t need = cg_conv2d_ups2_wino_wgrad_workspace_bytes(N, Hp, Wp, Cin, Cout);
    CG_REQUIRE(ws && ws_bytes >= need && (uintptr_t)ws % 16 == 0, "cg_conv2d_ups2_wino_wgrad: workspace too small (%zu < %zu)",
               ws_bytes, need);
    hipStream_t st = cg::S(stream);
    const int T = N * (Hp / 2) * (Wp / 2);
    const int C4 = 4 * Cout;
    char* base = (char*)ws;
    float* mdy = (float*)base;                    base += wino_align((size_t)16 * T * C4 * sizeof(float));
    float* dut = (float*)base;                    base += wino_align((size_t)16 * C4 * Cin * sizeof(float));
    void* bws = base;                             base += wino_bias_ws_bytes(Cout);
    void* tws = base;
    const size_t tws_bytes = ws_bytes - (size_t)(base - (char*)ws);
    hipLaunchKernelGGL(wino_dy_transform_kernel, dim3(cg::ew_grid((long)T * Cout)), dim3(256), 0, st, dy, mdy, N, Hp, Wp, Cout);
    CG_LAUNCH_CHECK();
    CG_HIP(hipMemsetAsync(dut, 0, (size_t)16 * C4 * Cin * sizeof(float), st));
    // 16 TN GEMMs dU_xi^T[pco][ci] = sum_tile Mdy_xi[tile][pco] V_xi[tile][ci]: the planes of V, Mdy and dU are equally spaced, so all
    // 16 run as ONE launch + one reduction (rounds 1-3: four launches of four)
    if (cg_conv2d_wgrad_strided(stream, 16, v, (long)T * Cin, mdy, (long)T * C4, dut, (long)C4 * Cin, T, 1, 1, Cin, C4, 1, 1, 0, 0, 0, 1.f,
                                tws, tws_bytes)) return 1;
    hipLaunchKernelGGL(wino_wgrad_finish_kernel, dim3(cg::ew_grid((long)Cout * Cin)), dim3(256), 0, st, dut, gw_canonical, Cout,
                       Cin, scale);
    CG_LAUNCH_CHECK();
    if (gb) return cg_bias_grad(stream, dy, gb, (long)N * 4 * Hp * Wp, Cout, scale, bws, wino_align(sizeof(double) * Cout));
    return 0;
}

}  // extern "C"
