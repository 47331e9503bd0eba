// The spatial transformer (stn: nn.AffineTransformMatrixGenerator, nn.AffineGridGeneratorBHWD, nn.BilinearSamplerBHWD): the affine
// matrix and grid with their gradients, the bilinear sampler and its deterministic gather backward.  NHWC fp32.
#include "common.h"

namespace {
using cg::block_sum_256;
using cg::Vec;

// The affine arithmetic itself (T, its gradient, the grid coordinate, the grid-gradient terms) is csrc/common.h's.
__global__ void affine_matrix_fwd_k(const float* params, float* T, int N, int ur, int us, int ut) {
    const int P = ur + us + 2 * ut;
    CG_GRID_STRIDE(n, N) cg::affine_T(params + (long)n * P, ur, us, ut, T + (long)n * 6);
}
__global__ void affine_matrix_bwd_k(const float* params, const float* gT, float* gparams, int N, int ur, int us, int ut) {
    const int P = ur + us + 2 * ut;
    CG_GRID_STRIDE(n, N) {
        float T[6], cs[5];
        cg::affine_T(params + (long)n * P, ur, us, ut, T, cs);
        cg::affine_param_grad(cs[0], cs[1], cs[2], cs[3], cs[4], gT + (long)n * 6, ur, us, ut, gparams + (long)n * P);
    }
}
__global__ void affine_grid_fwd_k(const float* T, float* grid, int N, int H, int W) {
    const long total = (long)N * H * W;
    CG_GRID_STRIDE(i, total) {
        const int j = (int)(i % W);
        long r = i / W;
        const int ii = (int)(r % H);
        const long n = r / H;
        const float y = cg::grid_coord(ii, H), x = cg::grid_coord(j, W);
        const float* t = T + n * 6;
        grid[i * 2 + 0] = t[0] * y + t[1] * x + t[2];
        grid[i * 2 + 1] = t[3] * y + t[4] * x + t[5];
    }
}
// one block per sample: gT[n][r][:] = sum_{i,j} ggrid[n,i,j,r] * (y_i, x_j, 1)
__global__ __launch_bounds__(256) void affine_grid_bwd_k(const float* ggrid, float* gT, int N, int H, int W) {
    __shared__ double sh[4];
    const int n = blockIdx.x;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const int HW = H * W;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const int ii = p / W, j = p - ii * W;
        cg::affine_grid_acc(acc, ggrid[((long)n * HW + p) * 2 + 0], ggrid[((long)n * HW + p) * 2 + 1], cg::grid_coord(ii, H), cg::grid_coord(j, W));
    }
    for (int k = 0; k < 6; ++k) {
        const double t = block_sum_256(acc[k], sh);
        if (threadIdx.x == 0) gT[(long)n * 6 + k] = (float)t;
    }
}

struct BilinTaps {
    int y0, x0;
    float wy0, wx0;  // weight of the top / left tap
    bool in00, in01, in10, in11;
};
__device__ __forceinline__ BilinTaps bilin_taps(float yf, float xf, int Hi, int Wi) {
    BilinTaps t;
    const float xc = (xf + 1.f) * (float)(Wi - 1) * 0.5f;
    const float yc = (yf + 1.f) * (float)(Hi - 1) * 0.5f;
    const float x0f = floorf(xc), y0f = floorf(yc);
    t.x0 = (int)x0f; t.y0 = (int)y0f;
    t.wx0 = 1.f - (xc - x0f);
    t.wy0 = 1.f - (yc - y0f);
    const bool xin0 = t.x0 >= 0 && t.x0 <= Wi - 1, xin1 = t.x0 + 1 >= 0 && t.x0 + 1 <= Wi - 1;
    const bool yin0 = t.y0 >= 0 && t.y0 <= Hi - 1, yin1 = t.y0 + 1 >= 0 && t.y0 + 1 <= Hi - 1;
    t.in00 = yin0 && xin0; t.in01 = yin0 && xin1; t.in10 = yin1 && xin0; t.in11 = yin1 && xin1;
    return t;
}
// Nimg: the image batch; sample n of the grid / output batch reads image n % Nimg (cg_bilinear_sampler_*_shared: G sibling
// transformers sampling the SAME images with their own grids, as one launch over G * Nimg samples)
// One lane per VW channels: VW = 4 where C % 4 == 0, the tensors are 16-byte aligned and the grid 8-byte (the taps are then derived once
// per four outputs), else 1; CV = C / VW.  Per channel the operations and their order do not depend on VW.
template <int VW>
__global__ __launch_bounds__(256) void bilinear_fwd_k(const float* __restrict__ img, const float* __restrict__ grid,
                                                      float* __restrict__ out, int N, int Nimg, int Hi, int Wi, int CV, int Ho, int Wo) {
    typedef Vec<VW> V;
    const long total = (long)N * Ho * Wo * CV;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % CV);
        const long pix = i / CV;
        const long n = (pix / ((long)Ho * Wo)) % Nimg;
        float gy = 0.f, gx = 0.f;
        if constexpr (VW == 4) { const float2 g = *reinterpret_cast<const float2*>(grid + pix * 2); gy = g.x; gx = g.y; }
        else { gy = grid[pix * 2]; gx = grid[pix * 2 + 1]; }
        const BilinTaps t = bilin_taps(gy, gx, Hi, Wi);
        const float* b = img + ((((n * Hi + t.y0) * (long)Wi + t.x0)) * CV + c) * VW;
        V v{V::zero()};
        auto tap = [&](bool in, float w, long off) {
            if (in) V::fma(v.v, w, V::ld(b + off * VW));
        };
        tap(t.in00, t.wx0 * t.wy0, 0);
        tap(t.in01, (1.f - t.wx0) * t.wy0, CV);
        tap(t.in10, t.wx0 * (1.f - t.wy0), (long)Wi * CV);
        tap(t.in11, (1.f - t.wx0) * (1.f - t.wy0), (long)Wi * CV + CV);
        v.store(out, i);
    }
}
// G lanes per output pixel (64/G pixels per wave), lanes stride the channels; G = smallest power of two >= min(C, 64)
template <int G>
__global__ __launch_bounds__(256) void bilinear_bwd_k(const float* img, const float* grid, const float* gout,
                                                      float* gimg, float* ggrid, int N, int Nimg, int Hi, int Wi, int C, int Ho,
                                                      int Wo) {
    const long npix = (long)N * Ho * Wo;
    const int sub = threadIdx.x & (G - 1);
    const long grp0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) / G;
    const long ngrp = ((long)gridDim.x * blockDim.x) / G;
    const long iters = (npix + ngrp - 1) / ngrp;   // same trip count for every lane of a wave (shuffles below)
    for (long it = 0; it < iters; ++it) {
        const long pix = grp0 + it * ngrp;
        const bool live = pix < npix;
        BilinTaps t;
        t.in00 = t.in01 = t.in10 = t.in11 = false; t.x0 = t.y0 = 0; t.wx0 = t.wy0 = 0.f;
        long n = 0;
        if (live) {
            n = pix / ((long)Ho * Wo);
            t = bilin_taps(grid[pix * 2], grid[pix * 2 + 1], Hi, Wi);
        }
        const long b = ((n * Hi + t.y0) * (long)Wi + t.x0) * C;
        const float* im = img + ((n % Nimg) - n) * (long)Hi * Wi * C;   // the image this sample reads (its own unless shared)
        const long o01 = C, o10 = (long)Wi * C, o11 = (long)Wi * C + C;
        float d00 = 0.f, d01 = 0.f, d10 = 0.f, d11 = 0.f;
        if (live)
            for (int c = sub; c < C; c += G) {
                const float g = gout[pix * C + c];
                if (t.in00) { d00 += im[b + c] * g;       atomicAdd(&gimg[b + c], t.wx0 * t.wy0 * g); }
                if (t.in01) { d01 += im[b + o01 + c] * g; atomicAdd(&gimg[b + o01 + c], (1.f - t.wx0) * t.wy0 * g); }
                if (t.in10) { d10 += im[b + o10 + c] * g; atomicAdd(&gimg[b + o10 + c], t.wx0 * (1.f - t.wy0) * g); }
                if (t.in11) { d11 += im[b + o11 + c] * g; atomicAdd(&gimg[b + o11 + c], (1.f - t.wx0) * (1.f - t.wy0) * g); }
            }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) {
            d00 += __shfl_down(d00, off, G); d01 += __shfl_down(d01, off, G);
            d10 += __shfl_down(d10, off, G); d11 += __shfl_down(d11, off, G);
        }
        if (live && sub == 0) {
            const float gy = -t.wx0 * d00 + t.wx0 * d10 - (1.f - t.wx0) * d01 + (1.f - t.wx0) * d11;
            const float gx = -t.wy0 * d00 + t.wy0 * d01 - (1.f - t.wy0) * d10 + (1.f - t.wy0) * d11;
            ggrid[pix * 2 + 0] = gy * (float)(Hi - 1) * 0.5f;
            ggrid[pix * 2 + 1] = gx * (float)(Wi - 1) * 0.5f;
        }
    }
}

// Deterministic backward (no float atomics): the reference pins this module to the CPU because stn's GPU scatter was
// "non-reproducible" (models.lua:889-899).  One workgroup = one sample x S pixel slots.  It stages the taps of ALL the
// sample's output pixels in LDS and buckets them by their top-left source cell (y0, x0) - counting sort with integer LDS
// atomics, every bucket then sorted by output-pixel index, so the bucket contents AND their order are reproducible.  Then
//   (A) for its S OUTPUT pixels: ggrid from the channel dot products (G lanes per pixel, sub-wave reduction), and
//   (B) for its S SOURCE pixels: gimg[q] = sum over the output pixels in the four buckets (y-1..y, x-1..x) that cover q,
//       in bucket order - a gather: every gimg element is written exactly once (no memset), in a fixed summation order.
// G = lanes per pixel (smallest power of two >= min(C, 64)); CACC = channels per lane.
// VW = floats per lane access: 4 when C % 4 == 0 and the tensors are 16-B aligned (a wave then covers 64 / G pixels with G = C / 4
// lanes each instead of one pixel per 64 channels), else 1.  A lane owns channels (sub + G * k) * VW .. + VW - 1.
template <int G, int CACC, int VW>
__global__ __launch_bounds__(256) void bilinear_bwd_det_k(const float* __restrict__ img, const float* __restrict__ grid,
                                                          const float* __restrict__ gout, float* __restrict__ gimg,
                                                          float* __restrict__ ggrid, int Nimg, int Hi, int Wi, int C, int Ho, int Wo,
                                                          int nchunks, int S) {
    extern __shared__ float bl_sh[];
    const int P = Ho * Wo, Q = Hi * Wi;
    const int CW = Wi + 1, NC = (Hi + 1) * CW;        // buckets: (y0 + 1, x0 + 1), y0 in [-1, Hi-1], x0 in [-1, Wi-1]
    int* ty0 = reinterpret_cast<int*>(bl_sh);
    int* tx0 = ty0 + P;
    float* twy = bl_sh + 2 * P;
    float* twx = bl_sh + 3 * P;
    int* list = reinterpret_cast<int*>(bl_sh) + 4 * P;  // [P] output pixels grouped by bucket
    int* cstart = list + P;                              // [NC + 1]
    int* ccnt = cstart + NC + 1;                         // [NC]
    __shared__ int part[256];
    const long n = blockIdx.x / nchunks;
    const int chunk = blockIdx.x % nchunks;
    const int tid = threadIdx.x;
    for (int c = tid; c < NC; c += 256) ccnt[c] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += 256) {
        const BilinTaps t = bilin_taps(grid[(n * P + p) * 2], grid[(n * P + p) * 2 + 1], Hi, Wi);
        ty0[p] = t.y0; tx0[p] = t.x0; twy[p] = t.wy0; twx[p] = t.wx0;
        if (t.y0 >= -1 && t.y0 <= Hi - 1 && t.x0 >= -1 && t.x0 <= Wi - 1) atomicAdd(&ccnt[(t.y0 + 1) * CW + t.x0 + 1], 1);
    }
    __syncthreads();
    // exclusive scan of the bucket counts: per-thread chunk sums, wave-level prefix sums of the 256 partials (shuffles) plus
    // the three wave totals, chunk-local offsets
    const int per = (NC + 255) / 256;
    int mine = 0;
    for (int c = tid * per; c < min(NC, (tid + 1) * per); ++c) mine += ccnt[c];
    {
        const int lane = tid & 63, wv = tid >> 6;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        __shared__ int wtot[4];
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wv; ++w) base += wtot[w];
        part[tid] = base + incl - mine;
        if (tid == 255) cstart[NC] = base + incl;
    }
    __syncthreads();
    {
        int run = part[tid];
        for (int c = tid * per; c < min(NC, (tid + 1) * per); ++c) { cstart[c] = run; run += ccnt[c]; ccnt[c] = 0; }
    }
    __syncthreads();
    for (int p = tid; p < P; p += 256) {
        const int y0 = ty0[p], x0 = tx0[p];
        if (y0 >= -1 && y0 <= Hi - 1 && x0 >= -1 && x0 <= Wi - 1) {
            const int c = (y0 + 1) * CW + x0 + 1;
            list[cstart[c] + atomicAdd(&ccnt[c], 1)] = p;    // arrival order is arbitrary ...
        }
    }
    __syncthreads();
    // ... so order every bucket by output-pixel index: an element's place is the number of smaller indices in its bucket (all threads, one
    // element each - a bucket is short unless the transformer collapses, and then P^2 / 256 broadcast reads per thread still bound it;
    // round 6: the insertion sort a single thread ran per bucket took 2-8 ms when every output pixel fell into one cell)
    int* sorted = ccnt + NC;                                 // [P]
    {
        const int placed = cstart[NC];
        for (int i = tid; i < placed; i += 256) {
            const int v = list[i];
            const int c = (ty0[v] + 1) * CW + tx0[v] + 1;
            const int b = cstart[c], e = b + ccnt[c];
            int rank = 0;
            for (int j = b; j < e; ++j) rank += list[j] < v ? 1 : 0;
            sorted[b + rank] = v;
        }
    }
    __syncthreads();
    list = sorted;
    const float* gsample = gout + n * (long)P * C;
    const float* isample = img + (n % Nimg) * (long)Q * C;
    const int sub = tid & (G - 1), grp = tid / G, ngrp = 256 / G;
    // ---- (A) grid gradient of this workgroup's output pixels (every lane of a wave runs the same trip count)
    for (int j0 = 0; j0 < S; j0 += ngrp) {
        const int p = chunk * S + j0 + grp;
        const bool live = j0 + grp < S && p < P;
        float d00 = 0.f, d01 = 0.f, d10 = 0.f, d11 = 0.f;
        float wy0 = 0.f, wx0 = 0.f;
        if (live) {
            const int y0 = ty0[p], x0 = tx0[p];
            wy0 = twy[p]; wx0 = twx[p];
            const bool xin0 = x0 >= 0 && x0 <= Wi - 1, xin1 = x0 + 1 >= 0 && x0 + 1 <= Wi - 1;
            const bool yin0 = y0 >= 0 && y0 <= Hi - 1, yin1 = y0 + 1 >= 0 && y0 + 1 <= Hi - 1;
            const long b = ((long)y0 * Wi + x0) * C;
            const long o01 = C, o10 = (long)Wi * C, o11 = (long)Wi * C + C;
#pragma unroll
            for (int k = 0; k < CACC; ++k) {
                const int c = (sub + G * k) * VW;
                if (c < C) {
                    typedef Vec<VW> V;
                    const typename V::T g = V::ld(gsample + (long)p * C + c);
                    const typename V::T i00 = (yin0 && xin0) ? V::ld(isample + b + c) : V::zero(), i01 = (yin0 && xin1) ? V::ld(isample + b + o01 + c) : V::zero();
                    const typename V::T i10 = (yin1 && xin0) ? V::ld(isample + b + o10 + c) : V::zero(), i11 = (yin1 && xin1) ? V::ld(isample + b + o11 + c) : V::zero();
                    d00 += V::dot(i00, g); d01 += V::dot(i01, g); d10 += V::dot(i10, g); d11 += V::dot(i11, g);
                }
            }
        }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) {
            d00 += __shfl_down(d00, off, G); d01 += __shfl_down(d01, off, G);
            d10 += __shfl_down(d10, off, G); d11 += __shfl_down(d11, off, G);
        }
        if (live && sub == 0) {
            const float gy = -wx0 * d00 + wx0 * d10 - (1.f - wx0) * d01 + (1.f - wx0) * d11;
            const float gx = -wy0 * d00 + wy0 * d01 - (1.f - wy0) * d10 + (1.f - wy0) * d11;
            ggrid[(n * P + p) * 2 + 0] = gy * (float)(Hi - 1) * 0.5f;
            ggrid[(n * P + p) * 2 + 1] = gx * (float)(Wi - 1) * 0.5f;
        }
    }
    // ---- (B) image gradient of this workgroup's source pixels
    constexpr int kHeavy = 64;                               // more taps than this on one source pixel: the whole workgroup sums them (below)
    __shared__ float coop[256 * CACC * VW];
    bool any_heavy = false;
    for (int j0 = 0; j0 < S; j0 += ngrp) {
        const int q = chunk * S + j0 + grp;
        if (!(j0 + grp < S && q < Q)) continue;
        const int y = q / Wi, x = q - y * Wi;
        // the four buckets whose 2x2 footprint contains (y, x): (y0, x0) = (y-1, x-1), (y-1, x), (y, x-1), (y, x)
        const int c00 = y * CW + x;                      // bucket index of (y0 = y-1, x0 = x-1)
        const int s0 = cstart[c00], n0 = ccnt[c00];
        const int s1 = cstart[c00 + 1], n1 = ccnt[c00 + 1];
        const int s2 = cstart[c00 + CW], n2 = ccnt[c00 + CW];
        const int s3 = cstart[c00 + CW + 1], n3 = ccnt[c00 + CW + 1];
        const int e1 = n0, e2 = n0 + n1, e3 = n0 + n1 + n2, total = e3 + n3;
        if (total > kHeavy) { any_heavy = true; continue; }
        typedef Vec<VW> V;
        typename V::T acc[CACC];
#pragma unroll
        for (int k = 0; k < CACC; ++k) acc[k] = V::zero();
        for (int i0 = 0; i0 < total; i0 += 4) {          // four gradient loads in flight, consumed in bucket order
            int ph[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u;
                if (i < total) {
                    const int e = i < e1 ? s0 + i : (i < e2 ? s1 + i - e1 : (i < e3 ? s2 + i - e2 : s3 + i - e3));
                    ph[u] = list[e];
                    const float wy = (y == ty0[ph[u]]) ? twy[ph[u]] : 1.f - twy[ph[u]];
                    const float wx = (x == tx0[ph[u]]) ? twx[ph[u]] : 1.f - twx[ph[u]];
                    w[u] = wx * wy;                       // same product order as the forward: (x weight) * (y weight)
                } else {
                    ph[u] = ph[0]; w[u] = 0.f;            // padding: adds an exact +0
                }
            }
            typename V::T g[4][CACC];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < CACC; ++k) {
                    const int c = (sub + G * k) * VW;
                    g[u][k] = c < C ? V::ld(gsample + (long)ph[u] * C + c) : V::zero();
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < CACC; ++k) V::fma(acc[k], w[u], g[u][k]);
        }
#pragma unroll
        for (int k = 0; k < CACC; ++k) {
            const int c = (sub + G * k) * VW;
            if (c < C) V::st(gimg + (n * Q + q) * C + c, acc[k]);
        }
    }
    // A source pixel under a collapsed transformer (scale -> 0: every output pixel samples the same cell) collects up to P taps; one lane
    // group summing them in a row is what made this kernel 75-750x slower there.  Such pixels are summed by the WHOLE workgroup: lane group r
    // takes the taps r, r + ngrp, ... in bucket order, the ngrp partial sums are added in group order - a fixed order again, so the result
    // is reproducible (it differs from the one-group order by fp32 re-association only, and only where more than kHeavy taps meet).
    if (__syncthreads_or(any_heavy ? 1 : 0)) {
        typedef Vec<VW> V;
        for (int j = 0; j < S; ++j) {
            const int q = chunk * S + j;
            if (q >= Q) break;
            const int y = q / Wi, x = q - y * Wi;
            const int c00 = y * CW + x;
            const int s0 = cstart[c00], n0 = ccnt[c00];
            const int s1 = cstart[c00 + 1], n1 = ccnt[c00 + 1];
            const int s2 = cstart[c00 + CW], n2 = ccnt[c00 + CW];
            const int s3 = cstart[c00 + CW + 1], n3 = ccnt[c00 + CW + 1];
            const int e1 = n0, e2 = n0 + n1, e3 = n0 + n1 + n2, total = e3 + n3;
            if (total <= kHeavy) continue;                // uniform over the workgroup
            typename V::T acc[CACC];
#pragma unroll
            for (int k = 0; k < CACC; ++k) acc[k] = V::zero();
            for (int i0 = grp; i0 < total; i0 += 2 * ngrp) {     // two loads in flight per lane group
                int ph[2];
                float w[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int i = i0 + u * ngrp;
                    if (i < total) {
                        const int e = i < e1 ? s0 + i : (i < e2 ? s1 + i - e1 : (i < e3 ? s2 + i - e2 : s3 + i - e3));
                        ph[u] = list[e];
                        const float wy = (y == ty0[ph[u]]) ? twy[ph[u]] : 1.f - twy[ph[u]];
                        const float wx = (x == tx0[ph[u]]) ? twx[ph[u]] : 1.f - twx[ph[u]];
                        w[u] = wx * wy;
                    } else {
                        ph[u] = ph[0]; w[u] = 0.f;
                    }
                }
                typename V::T g[2][CACC];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int k = 0; k < CACC; ++k) {
                        const int c = (sub + G * k) * VW;
                        g[u][k] = c < C ? V::ld(gsample + (long)ph[u] * C + c) : V::zero();
                    }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int k = 0; k < CACC; ++k) V::fma(acc[k], w[u], g[u][k]);
            }
            __syncthreads();                               // the previous heavy pixel's partial sums have been read
#pragma unroll
            for (int k = 0; k < CACC; ++k) V::st(coop + (tid * CACC + k) * VW, acc[k]);
            __syncthreads();
            if (grp == 0) {
                typename V::T tot[CACC];
#pragma unroll
                for (int k = 0; k < CACC; ++k) tot[k] = V::zero();
                for (int r = 0; r < ngrp; ++r)
#pragma unroll
                    for (int k = 0; k < CACC; ++k) V::fma(tot[k], 1.f, V::ld(coop + ((r * G + sub) * CACC + k) * VW));
#pragma unroll
                for (int k = 0; k < CACC; ++k) {
                    const int c = (sub + G * k) * VW;
                    if (c < C) V::st(gimg + (n * Q + q) * C + c, tot[k]);
                }
            }
        }
    }
}
}  // namespace

extern "C" {

int cg_affine_matrix_forward(void* stream, const float* params, float* T, int N, int use_rot, int use_scale,
                             int use_trans) {
    CG_REQUIRE(params && T, "cg_affine_matrix_forward: null pointer");
    CG_REQUIRE(use_rot || use_scale || use_trans, "cg_affine_matrix_forward: fully parametrised form not supported");
    CG_EW_LAUNCH(affine_matrix_fwd_k, (long)N, params, T, N, use_rot ? 1 : 0, use_scale ? 1 : 0, use_trans ? 1 : 0);
    return 0;
}
int cg_affine_matrix_backward(void* stream, const float* params, const float* gT, float* gparams, int N, int use_rot,
                              int use_scale, int use_trans) {
    CG_REQUIRE(params && gT && gparams, "cg_affine_matrix_backward: null pointer");
    CG_EW_LAUNCH(affine_matrix_bwd_k, (long)N, params, gT, gparams, N, use_rot ? 1 : 0, use_scale ? 1 : 0, use_trans ? 1 : 0);
    return 0;
}
int cg_affine_grid_forward(void* stream, const float* T, float* grid, int N, int H, int W) {
    CG_REQUIRE(T && grid, "cg_affine_grid_forward: null pointer");
    const long total = (long)N * H * W;
    CG_EW_LAUNCH(affine_grid_fwd_k, total, T, grid, N, H, W); return 0;
}
int cg_affine_grid_backward(void* stream, const float* ggrid, float* gT, int N, int H, int W) {
    CG_REQUIRE(ggrid && gT && N > 0, "cg_affine_grid_backward: bad args");
    hipLaunchKernelGGL(affine_grid_bwd_k, dim3(N), dim3(256), 0, cg::S(stream), ggrid, gT, N, H, W);
    CG_LAUNCH_CHECK(); return 0;
}
namespace {
int sampler_forward(void* stream, const float* img, const float* grid, float* out, int N, int Nimg, int Hi, int Wi, int C, int Ho,
                    int Wo) {
    const long total = (long)N * Ho * Wo * C;
    CG_EW_LAUNCH_V(cg::vec_ok(C, img, out) && (uintptr_t)grid % 8 == 0, bilinear_fwd_k<V>, total, img, grid, out, N, Nimg, Hi, Wi, C / V, Ho, Wo);
    return 0;
}

int sampler_backward(void* stream, const float* img, const float* grid, const float* gout, float* gimg, float* ggrid, int N, int Nimg,
                     int Hi, int Wi, int C, int Ho, int Wo) {
    const long P = (long)Ho * Wo, Q = (long)Hi * Wi;
    const size_t shb = ((size_t)6 * P + 2 * ((size_t)(Hi + 1) * (Wi + 1)) + 1) * 4;
    if (shb <= 140 * 1024 && C <= 256 && N > 0) {   // deterministic gather form
        const bool v4 = cg::vec_ok(C, img, gout, gimg);
        const int units = v4 ? C / 4 : C;                  // lane-sized channel units per pixel
        int G = 4;
        while (G < 64 && G < units) G <<= 1;
        // pixel slots per workgroup: at most 16 workgroups per sample (every workgroup stages and buckets all P taps again), and
        // no more workgroups than keep the chip busy (~4 per CU) when the batch is large
        const int want = std::max(1, std::min(16, (int)(cg::kNumCU * 4 / std::max(1, N))));
        const int S = std::max(std::max(32, 256 / G), cg::cdiv(std::max(P, Q), want));
        const int nchunks = cg::cdiv(std::max(P, Q), S);
        const dim3 grd((unsigned)((long)N * nchunks)), blk(256);
#define CG_BILIN_DET(GG, K, VV) hipLaunchKernelGGL((bilinear_bwd_det_k<GG, K, VV>), grd, blk, shb, cg::S(stream), img, grid, gout, gimg, ggrid, Nimg, Hi, Wi, C, Ho, Wo, nchunks, S)
        if (v4) {
            if (G == 4) CG_BILIN_DET(4, 1, 4);
            else if (G == 8) CG_BILIN_DET(8, 1, 4);
            else if (G == 16) CG_BILIN_DET(16, 1, 4);
            else if (G == 32) CG_BILIN_DET(32, 1, 4);
            else CG_BILIN_DET(64, 1, 4);                   // C <= 256
        } else if (G == 4) CG_BILIN_DET(4, 1, 1);
        else if (G == 8) CG_BILIN_DET(8, 1, 1);
        else if (G == 16) CG_BILIN_DET(16, 1, 1);
        else if (G == 32) CG_BILIN_DET(32, 1, 1);
        else if (C <= 64) CG_BILIN_DET(64, 1, 1);
        else if (C <= 128) CG_BILIN_DET(64, 2, 1);
        else CG_BILIN_DET(64, 4, 1);
#undef CG_BILIN_DET
        CG_LAUNCH_CHECK();
        return 0;
    }
    cg::opt_count(cg::OPT_SAMPLER_ATOMIC_LAUNCHES);
    CG_HIP(hipMemsetAsync(gimg, 0, sizeof(float) * (size_t)N * Hi * Wi * C, cg::S(stream)));
    const long npix = (long)N * Ho * Wo;
    int G = 4;
    while (G < 64 && G < C) G <<= 1;
    long blocks = (npix * G + 255) / 256;
    if (blocks > cg::kNumCU * 8) blocks = cg::kNumCU * 8;
    if (blocks < 1) blocks = 1;
    const dim3 grd((unsigned)blocks), blk(256);
#define CG_BILIN_BWD(GG) hipLaunchKernelGGL(bilinear_bwd_k<GG>, grd, blk, 0, cg::S(stream), img, grid, gout, gimg, ggrid, N, Nimg, Hi, Wi, C, Ho, Wo)
    switch (G) {
        case 4: CG_BILIN_BWD(4); break;
        case 8: CG_BILIN_BWD(8); break;
        case 16: CG_BILIN_BWD(16); break;
        case 32: CG_BILIN_BWD(32); break;
        default: CG_BILIN_BWD(64); break;
    }
#undef CG_BILIN_BWD
    CG_LAUNCH_CHECK(); return 0;
}
}  // namespace

int cg_bilinear_sampler_forward(void* stream, const float* img, const float* grid, float* out, int N, int Hi, int Wi,
                                int C, int Ho, int Wo) {
    CG_REQUIRE(img && grid && out && N > 0, "cg_bilinear_sampler_forward: null pointer");
    return sampler_forward(stream, img, grid, out, N, N, Hi, Wi, C, Ho, Wo);
}
int cg_bilinear_sampler_backward(void* stream, const float* img, const float* grid, const float* gout, float* gimg,
                                 float* ggrid, int N, int Hi, int Wi, int C, int Ho, int Wo) {
    CG_REQUIRE(img && grid && gout && gimg && ggrid && N > 0, "cg_bilinear_sampler_backward: null pointer");
    return sampler_backward(stream, img, grid, gout, gimg, ggrid, N, N, Hi, Wi, C, Ho, Wo);
}
int cg_bilinear_sampler_forward_shared(void* stream, int ngroups, const float* img, const float* grid, float* out, int N, int Hi,
                                       int Wi, int C, int Ho, int Wo) {
    CG_REQUIRE(img && grid && out && N > 0 && ngroups >= 1, "cg_bilinear_sampler_forward_shared: bad arguments");
    return sampler_forward(stream, img, grid, out, ngroups * N, N, Hi, Wi, C, Ho, Wo);
}
int cg_bilinear_sampler_backward_shared(void* stream, int ngroups, const float* img, const float* grid, const float* gout,
                                        float* gimg, float* ggrid, int N, int Hi, int Wi, int C, int Ho, int Wo) {
    CG_REQUIRE(img && grid && gout && gimg && ggrid && N > 0 && ngroups >= 1, "cg_bilinear_sampler_backward_shared: bad arguments");
    return sampler_backward(stream, img, grid, gout, gimg, ggrid, ngroups * N, N, Hi, Wi, C, Ho, Wo);
}
}  // extern "C"
