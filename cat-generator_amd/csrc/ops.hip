// The memory-bound operators of the G+D step that are neither a GEMM nor a subject of their own (runtime.hip, images.hip,
// sampler.hip, optim.hip, criterion.hip): activations, column reductions, batch-norm, pooling, dropout and its RNG, layout
// changes, small reductions.  NHWC fp32.  Each kernel cites the reference module it stands in for (see catgan.h).
#include "common.h"

namespace {
using cg::block_sum_256;
// ---------------------------------------------------------------- activations
// Memory-bound elementwise operators: one source each over cg::Vec<VW>.  VW = 4 moves 16 B per lane where the entry point finds
// cg::vec_ok() (n then counts float4s), VW = 1 is the scalar twin for the rest; a lane's arithmetic is cg::act / cg::dact of common.h.
using cg::Vec;

template <int VW>
__global__ void prelu_fwd_k(const float* x, const float* alpha, float* y, long n) {
    const float a = *alpha;
    CG_GRID_STRIDE(i, n) {
        Vec<VW> v = Vec<VW>::load(x, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = cg::act(1, v[k], a);
        v.store(y, i);
    }
}
// gpart[workgroup] = its sum over x <= 0 of x dy, for prelu_galpha_reduce_k
template <int VW>
__global__ void prelu_bwd_k(const float* x, const float* dy, const float* alpha, float* dx, double* gpart, long n) {
    cg::prelu_bwd_walk<VW>(x, dy, *alpha, dx, n, gpart ? gpart + blockIdx.x : nullptr);
}
// *galpha += scale * sum of the per-workgroup partials, in a fixed order (one same-address float atomic per
// workgroup costs ~12 ns each on this part: 25 us for a 2048-workgroup launch, and is order-dependent).  The scale is applied in
// fp64 and the product rounded once; galpha_groups_reduce_k (fused.hip) rounds the sum first and multiplies in fp32.
__global__ void prelu_galpha_reduce_k(const double* gpart, int nparts, float* galpha, float scale) {
    const double t = cg::partials_sum_256(gpart, nparts);
    if (threadIdx.x == 0) *galpha += (float)(t * scale);
}
template <int VW>
__global__ void lrelu_fwd_k(const float* x, float* y, float s, long n) {
    CG_GRID_STRIDE(i, n) {
        Vec<VW> v = Vec<VW>::load(x, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = cg::act(2, v[k], s);
        v.store(y, i);
    }
}
template <int VW>
__global__ void lrelu_bwd_k(const float* x, const float* dy, float* dx, float s, long n) {
    CG_GRID_STRIDE(i, n) {
        const Vec<VW> v = Vec<VW>::load(x, i);
        Vec<VW> g = Vec<VW>::load(dy, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) g[k] = cg::dact(2, v[k], g[k], s);
        g.store(dx, i);
    }
}
template <int VW>
__global__ void add_k(const float* a, const float* b, float* o, long n) {
    CG_GRID_STRIDE(i, n) {
        Vec<VW> u = Vec<VW>::load(a, i);
        const Vec<VW> v = Vec<VW>::load(b, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) u[k] += v[k];
        u.store(o, i);
    }
}
template <int VW>
__global__ void axpy_k(float al, const float* x, float* y, long n) {
    CG_GRID_STRIDE(i, n) {
        Vec<VW> v = Vec<VW>::load(y, i);
        Vec<VW>::fma(v.v, al, Vec<VW>::load(x, i).v);
        v.store(y, i);
    }
}
__global__ void sigmoid_fwd_k(const float* x, float* y, long n) {
    CG_GRID_STRIDE(i, n) { y[i] = 1.f / (1.f + expf(-x[i])); }
}
__global__ void sigmoid_bwd_k(const float* y, const float* dy, float* dx, long n) {
    CG_GRID_STRIDE(i, n) {
        const float v = y[i];
        dx[i] = dy[i] * (1.f - v) * v;
    }
}

// ------------------------------------------------------------- column reduces
// x: [M][C].  grid = (ceil(C/64), row chunks); block = 64 channels x 4 row lanes.
// MODE 0: (x, x^2)   MODE 1: (dy, dy*xhat)   MODE 2: (dy, 0)
template <int MODE>
__global__ __launch_bounds__(256) void colreduce_k(const float* x, const float* dy, const float* mean,
                                                   const float* invstd, long M, int C, long rows_per_block,
                                                   double* sums, cg::ColTree tree) {
    double* part = tree.part;
    __shared__ double sh1[4][64], sh2[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(M, r0 + rows_per_block);
    double a1 = 0.0, a2 = 0.0;
    if (c < C) {
        float s1 = 0.f, s2 = 0.f;
        float mu = 0.f, is = 0.f;
        if (MODE == 1) { mu = mean[c]; is = invstd[c]; }
        int cnt = 0;
        for (long r = r0 + rl; r < r1; r += 4) {
            const long i = r * C + c;
            if (MODE == 0) {
                const float v = x[i];
                s1 += v; s2 += v * v;
            } else if (MODE == 1) {
                const float g = dy[i];
                s1 += g; s2 += g * cg::bn_xhat(x[i], mu, is);
            } else {
                s1 += dy[i];
            }
            if (++cnt == 64) {  // bound fp32 partial length
                a1 += s1; a2 += s2; s1 = 0.f; s2 = 0.f; cnt = 0;
            }
        }
        a1 += s1; a2 += s2;
    }
    sh1[rl][cl] = a1; sh2[rl][cl] = a2;
    __syncthreads();
    if (rl == 0 && c < C) {
        const double t1 = sh1[0][cl] + sh1[1][cl] + sh1[2][cl] + sh1[3][cl];
        const double t2 = sh2[0][cl] + sh2[1][cl] + sh2[2][cl] + sh2[3][cl];
        const int nk = (MODE == 2 ? 1 : 2) * C;
        cg::st_agent(&part[(size_t)blockIdx.y * nk + c], t1);
        if (MODE != 2) cg::st_agent(&part[(size_t)blockIdx.y * nk + C + c], t2);
    }
    cg::col_tree_finish(tree, (int)blockIdx.y, (int)gridDim.y, gridDim.x, (MODE == 2 ? 1 : 2) * C, sums);
}

// float4 form (C % 4 == 0, 16-byte aligned rows): block = QB channel quads x RL row lanes (QB*RL = 256), four
// independent row loads in flight per thread, fp32 partials of <= 64 rows folded into doubles.
template <int MODE, int QB>
__global__ __launch_bounds__(256) void colreduce4_k(const float* x, const float* dy, const float* mean,
                                                    const float* invstd, long M, int C, long rows_per_block,
                                                    double* sums, cg::ColTree tree) {
    constexpr int RL = 256 / QB;
    double* part = tree.part;
    __shared__ double sh[2][RL][QB * 4 + 2];
    const int ql = threadIdx.x % QB, rl = threadIdx.x / QB;
    const int q = blockIdx.x * QB + ql;          // channel quad
    const int cq = C >> 2;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(M, r0 + rows_per_block);
    double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
    if (q < cq) {
        typedef Vec<4> V4;
        V4 mu{V4::zero()}, is = mu;
        if (MODE == 1) { mu = V4::ldc(mean, q); is = V4::ldc(invstd, q); }
        for (long rb = r0 + rl; rb < r1; rb += 64L * RL) {
            const long re = min(r1, rb + 64L * RL);
            V4 s1{V4::zero()}, s2 = s1;
#pragma unroll 4
            for (long r = rb; r < re; r += RL) {
                const long i = r * cq + q;
                if (MODE == 0) {
                    const V4 v = V4::load(x, i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) s1[k] += v[k];
#pragma unroll
                    for (int k = 0; k < 4; ++k) s2[k] += v[k] * v[k];
                } else {
                    const V4 g = V4::load(dy, i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) s1[k] += g[k];
                    if (MODE == 1) {
                        const V4 v = V4::load(x, i);
#pragma unroll
                        for (int k = 0; k < 4; ++k) s2[k] += g[k] * cg::bn_xhat(v[k], mu[k], is[k]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { a1[k] += s1[k]; a2[k] += s2[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { sh[0][rl][ql * 4 + k] = a1[k]; sh[1][rl][ql * 4 + k] = a2[k]; }
    __syncthreads();
    // 256 threads finish QB*4 channels x 2 sums
    for (int idx = threadIdx.x; idx < QB * 4 * (MODE == 2 ? 1 : 2); idx += 256) {
        const int which = idx / (QB * 4), cl = idx % (QB * 4);
        const int c = blockIdx.x * QB * 4 + cl;
        if (c >= C) continue;
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < RL; ++r) t += sh[which][r][cl];
        cg::st_agent(&part[(size_t)blockIdx.y * ((MODE == 2 ? 1 : 2) * C) + which * C + c], t);
    }
    cg::col_tree_finish(tree, (int)blockIdx.y, (int)gridDim.y, gridDim.x, (MODE == 2 ? 1 : 2) * C, sums);
}

__global__ void bias_grad_finish_k(const double* sums, float* gb, int C, float scale) {
    CG_GRID_STRIDE(c, C) { gb[c] += scale * (float)sums[c]; }
}

// --------------------------------------------------------------- batch-norm
__global__ void bn_prepare_k(const double* sums, double count, int C, float eps, float momentum, float* running_mean,
                             float* running_var, float* save_mean, float* save_invstd) {
    CG_GRID_STRIDE(c, C) {
        const double mean = sums[c] / count;
        double var = sums[C + c] / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        save_mean[c] = (float)mean;
        save_invstd[c] = invstd;
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
        if (running_var) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
        }
    }
}
// apply / backward over n lanes of VW channels (VW = 4: C % 4 == 0 and 16-byte aligned tensors), CV = C / VW
template <int VW>
__global__ void bn_apply_k(const float* x, float* y, const float* gamma, const float* beta, const float* mean,
                           const float* invstd, long n, int CV) {
    typedef Vec<VW> V;
    CG_GRID_STRIDE(i, n) {
        const int c = (int)(i % CV);
        const V g = V::ldc(gamma, c), b = V::ldc(beta, c), m = V::ldc(mean, c), s = V::ldc(invstd, c);
        V v = V::load(x, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = cg::bn_norm(v[k], m[k], s[k], g[k], b[k]);
        v.store(y, i);
    }
}
__global__ void bn_eval_k(const float* x, float* y, const float* gamma, const float* beta, const float* rm,
                          const float* rv, long total, int C, float eps) {
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        y[i] = (x[i] - rm[c]) / sqrtf(rv[c] + eps) * gamma[c] + beta[c];
    }
}
template <int VW>
__global__ void bn_bwd_k(const float* x, const float* dy, const float* gamma, const float* mean, const float* invstd,
                         const double* sums, double count, long n, int CV, float* dx) {
    typedef Vec<VW> V;
    const int C = CV * VW;
    CG_GRID_STRIDE(i, n) {
        const int c = (int)(i % CV);
        const V g = V::ldc(gamma, c), m = V::ldc(mean, c), s = V::ldc(invstd, c);
        const V v = V::load(x, i), d = V::load(dy, i);
        V o;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float m1 = (float)(sums[VW * c + k] / count), m2 = (float)(sums[C + VW * c + k] / count);
            o[k] = cg::bn_dx(v[k], d[k], g[k], m[k], s[k], m1, m2);
        }
        o.store(dx, i);
    }
}
__global__ void bn_bwd_param_k(const double* local_sums, int C, float* ggamma, float* gbeta, float scale) {
    CG_GRID_STRIDE(c, C) {
        if (gbeta) gbeta[c] += scale * (float)local_sums[c];
        if (ggamma) ggamma[c] += scale * (float)local_sums[C + c];
    }
}

// ------------------------------------------------------- resampling / pooling
__global__ void ups2_fwd_k(const float* x, float* y, int N, int H, int W, int C) {
    const long total = (long)N * 2 * H * 2 * W * C;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        long r = i / C;
        const int ox = (int)(r % (2 * W)); r /= (2 * W);
        const int oy = (int)(r % (2 * H));
        const long n = r / (2 * H);
        y[i] = x[((n * H + (oy >> 1)) * W + (ox >> 1)) * C + c];
    }
}
__global__ void ups2_bwd_k(const float* dy, float* dx, int N, int H, int W, int C) {
    const long total = (long)N * H * W * C;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        long r = i / C;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H);
        const long n = r / H;
        const long W2 = 2 * W;
        const long b = ((n * 2 * H + 2 * yy) * W2 + 2 * xx) * C + c;
        dx[i] = (dy[b] + dy[b + C]) + (dy[b + W2 * C] + dy[b + W2 * C + C]);
    }
}
template <bool MAX>
__global__ void pool2_fwd_k(const float* x, float* y, int N, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)N * Ho * Wo * C;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        long r = i / C;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long n = r / Ho;
        const long b = ((n * H + 2 * oy) * W + 2 * ox) * C + c;
        const float v00 = x[b], v01 = x[b + C], v10 = x[b + (long)W * C], v11 = x[b + (long)W * C + C];
        if (MAX) {
            float m = v00;
            if (v01 > m) m = v01;
            if (v10 > m) m = v10;
            if (v11 > m) m = v11;
            y[i] = m;
        } else {
            y[i] = (v00 + v01 + v10 + v11) * 0.25f;
        }
    }
}
__global__ void avgpool2_bwd_k(const float* dy, float* dx, int N, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)N * H * W * C;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        long r = i / C;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H);
        const long n = r / H;
        float v = 0.f;
        if ((yy >> 1) < Ho && (xx >> 1) < Wo) v = dy[((n * Ho + (yy >> 1)) * Wo + (xx >> 1)) * C + c] * 0.25f;
        dx[i] = v;
    }
}
__global__ void maxpool2_bwd_k(const float* x, const float* dy, float* dx, int N, int H, int W, int C) {
    // one thread per pooled output: route the gradient to the first max in scan order
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)N * Ho * Wo * C;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        long r = i / C;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long n = r / Ho;
        const long b = ((n * H + 2 * oy) * W + 2 * ox) * C + c;
        const long o01 = C, o10 = (long)W * C, o11 = (long)W * C + C;
        const float v00 = x[b], v01 = x[b + o01], v10 = x[b + o10], v11 = x[b + o11];
        int arg = 0; float m = v00;
        if (v01 > m) { m = v01; arg = 1; }
        if (v10 > m) { m = v10; arg = 2; }
        if (v11 > m) { m = v11; arg = 3; }
        const float g = dy[i];
        dx[b] = arg == 0 ? g : 0.f;
        dx[b + o01] = arg == 1 ? g : 0.f;
        dx[b + o10] = arg == 2 ? g : 0.f;
        dx[b + o11] = arg == 3 ? g : 0.f;
    }
}

// -------------------------------------------------------------------- dropout
// y = x * mask over n lanes of VW floats.  SPATIAL: mask[sample][channel] (CV = C / VW, HWCV lanes per sample; VW = 4 needs C % 4 == 0,
// the mask itself any alignment), else a full-size mask (VW = 4: 16-byte aligned)
template <int VW, bool SPATIAL>
__global__ void mask_mul_k(const float* x, const float* mask, float* y, long n, long HWCV, int CV) {
    typedef Vec<VW> V;
    CG_GRID_STRIDE(i, n) {
        const V m = SPATIAL ? V::ldc(mask, (int)((i / HWCV) * CV + (i % CV))) : V::load(mask, i);
        V v = V::load(x, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] *= m[k];
        v.store(y, i);
    }
}
using cg::u01;
__global__ void rng_bernoulli_k(float* out, long n, float keep, float value, uint64_t seed, uint64_t offset,
                                const uint64_t* base) {
    if (base) offset += *base;
    CG_GRID_STRIDE(i, n) { out[i] = u01(seed, offset + (uint64_t)i) < keep ? value : 0.f; }
}
__global__ void rng_uniform_k(float* out, long n, float lo, float hi, uint64_t seed, uint64_t offset,
                              const uint64_t* base) {
    if (base) offset += *base;
    CG_GRID_STRIDE(i, n) { out[i] = lo + (hi - lo) * u01(seed, offset + (uint64_t)i); }
}
__global__ void rng_randint_k(int32_t* out, long n, int32_t range, uint64_t seed, uint64_t offset, const uint64_t* base) {
    if (base) offset += *base;
    CG_GRID_STRIDE(i, n) {
        int32_t v = (int32_t)(u01(seed, offset + (uint64_t)i) * (float)range);
        out[i] = v < range ? v : range - 1;
    }
}
// G consecutive blocks of n floats, block g drawn at its own position off<g> of the counter stream (the dropout masks of
// D32_st3's identical branches, which a branch-after-branch walk would draw at different positions)
__global__ void rng_bernoulli_groups_k(float* out, long n, int G, float keep, float value, uint64_t seed, uint64_t off0,
                                       uint64_t off1, uint64_t off2, uint64_t off3, const uint64_t* base) {
    const uint64_t b = base ? *base : 0ull;
    CG_GRID_STRIDE(i, n * G) {
        const int g = (int)(i / n);
        const uint64_t off = g == 0 ? off0 : (g == 1 ? off1 : (g == 2 ? off2 : off3));
        out[i] = u01(seed, b + off + (uint64_t)(i - (long)g * n)) < keep ? value : 0.f;
    }
}
__global__ void counter_add_k(uint64_t* c, uint64_t d) { if (threadIdx.x == 0 && blockIdx.x == 0) *c += d; }

// --------------------------------------------------------------------- layout
__global__ void nchw_to_nhwc_k(const float* in, float* out, int N, int C, int H, int W) {
    const long total = (long)N * C * H * W;
    CG_GRID_STRIDE(i, total) {  // i indexes the NHWC output
        const int c = (int)(i % C);
        long r = i / C;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const long n = r / H;
        out[i] = in[((n * C + c) * H + y) * W + x];
    }
}
__global__ void nhwc_to_nchw_k(const float* in, float* out, int N, int C, int H, int W) {
    const long total = (long)N * C * H * W;
    CG_GRID_STRIDE(i, total) {  // i indexes the NCHW output
        const int x = (int)(i % W);
        long r = i / W;
        const int y = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const long n = r / C;
        out[i] = in[((n * H + y) * W + x) * C + c];
    }
}
__global__ void copy_channels_k(const float* src, float* dst, long M, int Csrc, int so, int Cdst, int dof, int Cc) {
    const long total = M * Cc;
    CG_GRID_STRIDE(i, total) {
        const int c = (int)(i % Cc);
        const long m = i / Cc;
        dst[m * Cdst + dof + c] = src[m * Csrc + so + c];
    }
}
__global__ void gather_rows_k(const float* src, const int32_t* idx, float* dst, long nrows, long rowlen) {
    const long total = nrows * rowlen;
    CG_GRID_STRIDE(i, total) {
        const long r = i / rowlen, j = i - r * rowlen;
        dst[i] = src[(long)idx[r] * rowlen + j];
    }
}
__global__ void fill_k(float* x, float v, long n) { CG_GRID_STRIDE(i, n) x[i] = v; }
__global__ void axpy_sign_k(float al, const float* x, float* y, long n) {
    CG_GRID_STRIDE(i, n) {
        const float v = x[i];
        y[i] += al * (v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f));
    }
}
__global__ void scale_k(float* x, float al, long n) { CG_GRID_STRIDE(i, n) x[i] *= al; }
__global__ void clamp_k(float* x, float lo, float hi, long n) {
    CG_GRID_STRIDE(i, n) { x[i] = fminf(fmaxf(x[i], lo), hi); }
}
template <bool SQ>
__global__ void sumred_k(const float* x, long n, double* out) {
    __shared__ double sh[4];
    double s = 0.0;
    CG_GRID_STRIDE(i, n) {
        const float v = x[i];
        s += SQ ? (double)v * (double)v : (double)fabsf(v);
    }
    const double t = block_sum_256(s, sh);
    if (threadIdx.x == 0) atomicAdd(out, t);
}
__global__ void confusion_k(const float* out, const float* tgt, int32_t* counts, long n) {
    CG_GRID_STRIDE(i, n) {
        const int pred = out[i] > 0.5f ? 1 : 0;
        const int t = tgt[i] > 0.5f ? 1 : 0;
        atomicAdd(&counts[pred * 2 + t], 1);
    }
}

}  // namespace

extern "C" {

int cg_prelu_forward(void* stream, const float* x, const float* alpha, float* y, long n) {
    CG_REQUIRE(x && alpha && y, "cg_prelu_forward: null pointer");
    CG_EW_LAUNCH_V(cg::vec_ok(n, x, y), prelu_fwd_k<V>, n, x, alpha, y, n / V);
    return 0;
}
size_t cg_prelu_backward_workspace_bytes(long n) { return n > 0 ? sizeof(double) * (size_t)cg::ew_grid(n) : 0; }
int cg_prelu_backward(void* stream, const float* x, const float* dy, const float* alpha, float* dx, float* galpha,
                      float scale, long n, void* ws, size_t ws_bytes) {
    CG_REQUIRE(x && dy && alpha && dx, "cg_prelu_backward: null pointer");
    if (n <= 0) return 0;
    const bool v4 = cg::vec_ok(n, x, dy, dx);
    const int nblk = cg::ew_grid(v4 ? n / 4 : n);
    double* gpart = nullptr;
    if (galpha) {
        CG_REQUIRE(ws && ws_bytes >= sizeof(double) * nblk && ((uintptr_t)ws % 8) == 0,
                   "cg_prelu_backward: workspace too small (%zu < %zu)", ws_bytes, sizeof(double) * nblk);
        gpart = (double*)ws;
    }
    CG_EW_LAUNCH_V(v4, prelu_bwd_k<V>, n, x, dy, alpha, dx, gpart, n / V);
    if (galpha) {
        hipLaunchKernelGGL(prelu_galpha_reduce_k, dim3(1), dim3(256), 0, cg::S(stream), gpart, nblk, galpha, scale);
        CG_LAUNCH_CHECK();
    }
    return 0;
}
int cg_leakyrelu_forward(void* stream, const float* x, float* y, float slope, long n) {
    CG_REQUIRE(x && y, "cg_leakyrelu_forward: null pointer");
    CG_EW_LAUNCH_V(cg::vec_ok(n, x, y), lrelu_fwd_k<V>, n, x, y, slope, n / V);
    return 0;
}
int cg_leakyrelu_backward(void* stream, const float* x, const float* dy, float* dx, float slope, long n) {
    CG_REQUIRE(x && dy && dx, "cg_leakyrelu_backward: null pointer");
    CG_EW_LAUNCH_V(cg::vec_ok(n, x, dy, dx), lrelu_bwd_k<V>, n, x, dy, dx, slope, n / V);
    return 0;
}
int cg_sigmoid_forward(void* stream, const float* x, float* y, long n) {
    CG_REQUIRE(x && y, "cg_sigmoid_forward: null pointer");
    CG_EW_LAUNCH(sigmoid_fwd_k, n, x, y, n); return 0;
}
int cg_sigmoid_backward(void* stream, const float* y, const float* dy, float* dx, long n) {
    CG_REQUIRE(y && dy && dx, "cg_sigmoid_backward: null pointer");
    CG_EW_LAUNCH(sigmoid_bwd_k, n, y, dy, dx, n); return 0;
}
static int colreduce_launch(void* stream, int mode, const float* x, const float* dy, const float* mean,
                            const float* invstd, long M, int C, double* sums, int nsums) {
    if (M <= 0) { CG_HIP(hipMemsetAsync(sums, 0, sizeof(double) * nsums * C, cg::S(stream))); return 0; }
    const bool v4 = cg::vec_ok(C, x, dy);
    const int qb = C >= 128 ? 32 : 16;   // channel quads per block in the float4 form
    const int cblocks = v4 ? cg::cdiv(C / 4, qb) : cg::cdiv(C, 64);
    // row chunks: every chunk ends in one double atomic per channel, and same-address atomics serialise (~10 ns each),
    // so aim at one workgroup per CU in total (CG_COLREDUCE_WGS_PER_CU) rather than at maximum occupancy
    const int cmul = cg::kColReduceWgsPerCU;
    long chunks = std::max(1L, std::min((M + 63) / 64, (long)cg::kNumCU * cmul / cblocks));
    const long rows_per_block = ((M + chunks - 1) / chunks + 3) / 4 * 4;
    chunks = (M + rows_per_block - 1) / rows_per_block;
    dim3 grid(cblocks, (unsigned)chunks);
    // deterministic sum inside one launch: partials in the stream's scratch, added in a fixed two-level order (cg::ColTree)
    char* scr = (char*)cg::col_scratch(cg::S(stream));
    if (!scr) return 1;
    cg::ColTree tree;
    CG_REQUIRE(cg::col_tree_layout(scr, chunks, (size_t)nsums * C, 0, tree), "column reduce: %ld chunks x %d sums exceed the scratch", chunks, nsums * C);
#define CG_COLRED(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, cg::S(stream), x, dy, mean, invstd, M, C, rows_per_block, sums, tree)
    if (v4 && qb == 32) {
        if (mode == 0) CG_COLRED((colreduce4_k<0, 32>)); else if (mode == 1) CG_COLRED((colreduce4_k<1, 32>)); else CG_COLRED((colreduce4_k<2, 32>));
    } else if (v4) {
        if (mode == 0) CG_COLRED((colreduce4_k<0, 16>)); else if (mode == 1) CG_COLRED((colreduce4_k<1, 16>)); else CG_COLRED((colreduce4_k<2, 16>));
    } else {
        if (mode == 0) CG_COLRED(colreduce_k<0>); else if (mode == 1) CG_COLRED(colreduce_k<1>); else CG_COLRED(colreduce_k<2>);
    }
#undef CG_COLRED
    CG_LAUNCH_CHECK();
    return 0;
}

int cg_bias_grad(void* stream, const float* dy, float* gb, long M, int C, float scale, void* ws, size_t ws_bytes) {
    CG_REQUIRE(dy && gb && C > 0, "cg_bias_grad: bad args");
    CG_REQUIRE(ws && ws_bytes >= sizeof(double) * (size_t)C, "cg_bias_grad: workspace too small");
    double* scratch = (double*)ws;
    if (colreduce_launch(stream, 2, nullptr, dy, nullptr, nullptr, M, C, scratch, 1)) return 1;
    CG_EW_LAUNCH(bias_grad_finish_k, (long)C, (const double*)scratch, gb, C, scale);
    return 0;
}

int cg_bn_stats(void* stream, const float* x, long M, int C, double* sums) {
    CG_REQUIRE(x && sums && C > 0, "cg_bn_stats: bad args");
    return colreduce_launch(stream, 0, x, nullptr, nullptr, nullptr, M, C, sums, 2);
}
int cg_bn_forward(void* stream, const float* x, float* y, const float* gamma, const float* beta, const double* sums,
                  double count, long M, int C, float eps, float momentum, float* running_mean, float* running_var,
                  float* save_mean, float* save_invstd) {
    CG_REQUIRE(x && y && gamma && beta && sums && save_mean && save_invstd && C > 0 && count > 0, "cg_bn_forward: bad args");
    CG_EW_LAUNCH(bn_prepare_k, (long)C, sums, count, C, eps, momentum, running_mean, running_var, save_mean, save_invstd);
    const long total = M * C;
    CG_EW_LAUNCH_V(cg::vec_ok(C, x, y), bn_apply_k<V>, total, x, y, gamma, beta, (const float*)save_mean, (const float*)save_invstd, total / V, C / V);
    return 0;
}
int cg_bn_forward_eval(void* stream, const float* x, float* y, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, long M, int C, float eps) {
    CG_REQUIRE(x && y && gamma && beta && running_mean && running_var && C > 0, "cg_bn_forward_eval: bad args");
    const long total = M * C;
    CG_EW_LAUNCH(bn_eval_k, total, x, y, gamma, beta, running_mean, running_var, total, C, eps);
    return 0;
}
int cg_bn_backward_stats(void* stream, const float* x, const float* dy, const float* save_mean, const float* save_invstd,
                         long M, int C, double* sums) {
    CG_REQUIRE(x && dy && save_mean && save_invstd && sums && C > 0, "cg_bn_backward_stats: bad args");
    return colreduce_launch(stream, 1, x, dy, save_mean, save_invstd, M, C, sums, 2);
}
int cg_bn_backward(void* stream, const float* x, const float* dy, const float* gamma, const float* save_mean,
                   const float* save_invstd, const double* sums, double count, const double* local_sums, long M, int C,
                   float* dx, float* ggamma, float* gbeta, float scale) {
    CG_REQUIRE(x && dy && gamma && save_mean && save_invstd && sums && local_sums && dx && C > 0 && count > 0,
               "cg_bn_backward: bad args");
    const long total = M * C;
    CG_EW_LAUNCH_V(cg::vec_ok(C, x, dy, dx), bn_bwd_k<V>, total, x, dy, gamma, save_mean, save_invstd, sums, count, total / V, C / V, dx);
    CG_EW_LAUNCH(bn_bwd_param_k, (long)C, local_sums, C, ggamma, gbeta, scale);
    return 0;
}

int cg_upsample2x_forward(void* stream, const float* x, float* y, int N, int H, int W, int C) {
    CG_REQUIRE(x && y, "cg_upsample2x_forward: null pointer");
    const long total = (long)N * 4 * H * W * C;
    CG_EW_LAUNCH(ups2_fwd_k, total, x, y, N, H, W, C); return 0;
}
int cg_upsample2x_backward(void* stream, const float* dy, float* dx, int N, int H, int W, int C) {
    CG_REQUIRE(dy && dx, "cg_upsample2x_backward: null pointer");
    const long total = (long)N * H * W * C;
    CG_EW_LAUNCH(ups2_bwd_k, total, dy, dx, N, H, W, C); return 0;
}
int cg_avgpool2_forward(void* stream, const float* x, float* y, int N, int H, int W, int C) {
    CG_REQUIRE(x && y, "cg_avgpool2_forward: null pointer");
    const long total = (long)N * (H / 2) * (W / 2) * C;
    CG_EW_LAUNCH(pool2_fwd_k<false>, total, x, y, N, H, W, C); return 0;
}
int cg_avgpool2_backward(void* stream, const float* dy, float* dx, int N, int H, int W, int C) {
    CG_REQUIRE(dy && dx, "cg_avgpool2_backward: null pointer");
    const long total = (long)N * H * W * C;
    CG_EW_LAUNCH(avgpool2_bwd_k, total, dy, dx, N, H, W, C); return 0;
}
int cg_maxpool2_forward(void* stream, const float* x, float* y, int N, int H, int W, int C) {
    CG_REQUIRE(x && y, "cg_maxpool2_forward: null pointer");
    const long total = (long)N * (H / 2) * (W / 2) * C;
    CG_EW_LAUNCH(pool2_fwd_k<true>, total, x, y, N, H, W, C); return 0;
}
int cg_maxpool2_backward(void* stream, const float* x, const float* dy, float* dx, int N, int H, int W, int C) {
    CG_REQUIRE(x && dy && dx, "cg_maxpool2_backward: null pointer");
    CG_REQUIRE(H % 2 == 0 && W % 2 == 0, "cg_maxpool2_backward: odd spatial size");
    const long total = (long)N * (H / 2) * (W / 2) * C;
    CG_EW_LAUNCH(maxpool2_bwd_k, total, x, dy, dx, N, H, W, C); return 0;
}
int cg_mask_mul(void* stream, const float* x, const float* mask, float* y, int N, long HW, int C, int spatial) {
    CG_REQUIRE(x && mask && y, "cg_mask_mul: null pointer");
    const long total = (long)N * HW * C;
    // three forms: a [N][C] mask with C % 4 == 0, a full-size aligned mask with total % 4 == 0, and the scalar kernel for the rest
    const bool v4 = spatial ? cg::vec_ok(C, x, y) : cg::vec_ok(total, x, y, mask);
    if (spatial) CG_EW_LAUNCH_V(v4, (mask_mul_k<V, true>), total, x, mask, y, total / V, HW * C / V, C / V);
    else CG_EW_LAUNCH_V(v4, (mask_mul_k<V, false>), total, x, mask, y, total / V, 0L, 0);
    return 0;
}
int cg_rng_bernoulli_dev(void* stream, float* out, long n, float keep_prob, float value, uint64_t seed, uint64_t offset,
                         const uint64_t* base) {
    CG_REQUIRE(out, "cg_rng_bernoulli: null pointer");
    CG_EW_LAUNCH(rng_bernoulli_k, n, out, n, keep_prob, value, seed, offset, base); return 0;
}
int cg_rng_bernoulli_dev_grouped(void* stream, float* out, long n_per_group, int ngroups, float keep_prob, float value,
                                 uint64_t seed, uint64_t off0, uint64_t off1, uint64_t off2, uint64_t off3,
                                 const uint64_t* base) {
    CG_REQUIRE(out && ngroups >= 1 && ngroups <= 4, "cg_rng_bernoulli_dev_grouped: bad args");
    CG_EW_LAUNCH(rng_bernoulli_groups_k, n_per_group * ngroups, out, n_per_group, ngroups, keep_prob, value, seed, off0, off1, off2,
              off3, base);
    return 0;
}
int cg_rng_uniform_dev(void* stream, float* out, long n, float lo, float hi, uint64_t seed, uint64_t offset,
                       const uint64_t* base) {
    CG_REQUIRE(out, "cg_rng_uniform: null pointer");
    CG_EW_LAUNCH(rng_uniform_k, n, out, n, lo, hi, seed, offset, base); return 0;
}
int cg_rng_randint_dev(void* stream, int32_t* out, long n, int32_t range, uint64_t seed, uint64_t offset,
                       const uint64_t* base) {
    CG_REQUIRE(out && range > 0, "cg_rng_randint: bad args");
    CG_EW_LAUNCH(rng_randint_k, n, out, n, range, seed, offset, base); return 0;
}
int cg_rng_bernoulli(void* stream, float* out, long n, float keep_prob, float value, uint64_t seed, uint64_t offset) {
    return cg_rng_bernoulli_dev(stream, out, n, keep_prob, value, seed, offset, nullptr);
}
int cg_rng_uniform(void* stream, float* out, long n, float lo, float hi, uint64_t seed, uint64_t offset) {
    return cg_rng_uniform_dev(stream, out, n, lo, hi, seed, offset, nullptr);
}
int cg_rng_randint(void* stream, int32_t* out, long n, int32_t range, uint64_t seed, uint64_t offset) {
    return cg_rng_randint_dev(stream, out, n, range, seed, offset, nullptr);
}
int cg_counter_add(void* stream, uint64_t* counter, uint64_t delta) {
    CG_REQUIRE(counter, "cg_counter_add: null pointer");
    hipLaunchKernelGGL(counter_add_k, dim3(1), dim3(64), 0, cg::S(stream), counter, delta);
    CG_LAUNCH_CHECK(); return 0;
}
int cg_nchw_to_nhwc(void* stream, const float* in, float* out, int N, int C, int H, int W) {
    CG_REQUIRE(in && out, "cg_nchw_to_nhwc: null pointer");
    const long total = (long)N * C * H * W;
    CG_EW_LAUNCH(nchw_to_nhwc_k, total, in, out, N, C, H, W); return 0;
}
int cg_nhwc_to_nchw(void* stream, const float* in, float* out, int N, int C, int H, int W) {
    CG_REQUIRE(in && out, "cg_nhwc_to_nchw: null pointer");
    const long total = (long)N * C * H * W;
    CG_EW_LAUNCH(nhwc_to_nchw_k, total, in, out, N, C, H, W); return 0;
}
int cg_copy_channels(void* stream, const float* src, float* dst, long M, int Csrc, int src_off, int Cdst, int dst_off,
                     int Ccopy) {
    CG_REQUIRE(src && dst, "cg_copy_channels: null pointer");
    CG_REQUIRE(src_off >= 0 && dst_off >= 0 && src_off + Ccopy <= Csrc && dst_off + Ccopy <= Cdst,
               "cg_copy_channels: slice out of range");
    const long total = M * Ccopy;
    CG_EW_LAUNCH(copy_channels_k, total, src, dst, M, Csrc, src_off, Cdst, dst_off, Ccopy); return 0;
}
int cg_gather_rows(void* stream, const float* src, const int32_t* idx, float* dst, long nrows, long rowlen) {
    CG_REQUIRE(src && idx && dst, "cg_gather_rows: null pointer");
    const long total = nrows * rowlen;
    CG_EW_LAUNCH(gather_rows_k, total, src, idx, dst, nrows, rowlen); return 0;
}
int cg_fill(void* stream, float* x, float value, long n) {
    CG_REQUIRE(x, "cg_fill: null pointer");
    CG_EW_LAUNCH(fill_k, n, x, value, n); return 0;
}
int cg_add(void* stream, const float* a, const float* b, float* out, long n) {
    CG_REQUIRE(a && b && out, "cg_add: null pointer");
    CG_EW_LAUNCH_V(cg::vec_ok(n, a, b, out), add_k<V>, n, a, b, out, n / V);
    return 0;
}
int cg_axpy(void* stream, float alpha, const float* x, float* y, long n) {
    CG_REQUIRE(x && y, "cg_axpy: null pointer");
    CG_EW_LAUNCH_V(cg::vec_ok(n, x, y), axpy_k<V>, n, alpha, x, y, n / V);
    return 0;
}
int cg_axpy_sign(void* stream, float alpha, const float* x, float* y, long n) {
    CG_REQUIRE(x && y, "cg_axpy_sign: null pointer");
    CG_EW_LAUNCH(axpy_sign_k, n, alpha, x, y, n); return 0;
}
int cg_scale(void* stream, float* x, float alpha, long n) {
    CG_REQUIRE(x, "cg_scale: null pointer");
    CG_EW_LAUNCH(scale_k, n, x, alpha, n); return 0;
}
int cg_clamp(void* stream, float* x, float lo, float hi, long n) {
    CG_REQUIRE(x, "cg_clamp: null pointer");
    CG_EW_LAUNCH(clamp_k, n, x, lo, hi, n); return 0;
}
int cg_sumsq(void* stream, const float* x, long n, double* out) {
    CG_REQUIRE(x && out, "cg_sumsq: null pointer");
    CG_HIP(hipMemsetAsync(out, 0, sizeof(double), cg::S(stream)));
    CG_EW_LAUNCH(sumred_k<true>, n, x, n, out); return 0;
}
int cg_sumabs(void* stream, const float* x, long n, double* out) {
    CG_REQUIRE(x && out, "cg_sumabs: null pointer");
    CG_HIP(hipMemsetAsync(out, 0, sizeof(double), cg::S(stream)));
    CG_EW_LAUNCH(sumred_k<false>, n, x, n, out); return 0;
}
int cg_confusion_update(void* stream, const float* outputs, const float* targets, int32_t* counts, long n) {
    CG_REQUIRE(outputs && targets && counts, "cg_confusion_update: null pointer");
    CG_EW_LAUNCH(confusion_k, n, outputs, targets, counts, n); return 0;
}

}  // extern "C"
