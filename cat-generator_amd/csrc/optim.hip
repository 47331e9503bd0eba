// The optimisers, one pass over the flat parameter vector each: penalty + clamp + Adam, the same with the running average of the
// parameters (--G_ema) in the pass, the average alone, SGD and Adagrad.
#include "common.h"

namespace {
// penalty + clamp + Adam on one element, written once: adam_k and adam_ema_k (both widths) evaluate this and nothing else.  Every
// product and sum below is rounded on its own - the code adam_k has always compiled to (packed multiplies and adds, no fma) - and
// the pragma makes that the source's statement instead of the compiler's choice: with contraction allowed, the float4 kernel
// fuses b1 * m into the sum and moves m by an ulp against the scalar one.  The penalty is adam's own text, not pen_clamp below:
// sgd_k and adagrad_k keep the form (and the bits) they compile to.
__device__ __forceinline__ void adam_elem(float& pi, float& gi, float& mi, float& vi, float step, float b1, float b2, float eps,
                                          float l1, float l2, float clampv) {
#pragma clang fp contract(off)
    if (l1 != 0.f || l2 != 0.f) {
        const float sg = pi > 0.f ? 1.f : (pi < 0.f ? -1.f : 0.f);
        gi += sg * l1 + pi * l2;
    }
    if (clampv > 0.f) gi = fminf(fmaxf(gi, -clampv), clampv);
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    pi = pi - step * mi / (sqrtf(vi) + eps);
}
// replay-safe bias correction from the device-side step counter
__device__ __forceinline__ float adam_step_dev(float lr, float b1, float b2, const uint64_t* t_dev) {
    const double t = (double)*t_dev;
    return (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
}
__global__ void adam_k(float* p, float* g, float* m, float* v, long n, float step, float b1, float b2, float eps,
                       float l1, float l2, float clampv, int write_back, float lr, const uint64_t* t_dev) {
    if (t_dev) step = adam_step_dev(lr, b1, b2, t_dev);
    CG_GRID_STRIDE(i, n) {
        float pi = p[i], gi = g[i], mi = m[i], vi = v[i];
        adam_elem(pi, gi, mi, vi, step, b1, b2, eps, l1, l2, clampv);
        m[i] = mi; v[i] = vi;
        p[i] = pi;
        if (write_back) g[i] = gi;
    }
}
// ---- running average of the parameters (--G_ema): e = d e + (1 - d) p', the product rounded on its own, then one fma.  Written once and
// spelled with intrinsics, so that the contraction the build allows cannot pick another form in another kernel.  omd = 1.f - d.
__device__ __forceinline__ float ema_elem(float e, float p, float d, float omd) { return fmaf(d, e, __fmul_rn(omd, p)); }
// d_n = (float) min((double)cap, (1 + n) / (10 + n)) from the device-side count of applied updates: the double expression
// optim.ema_decay evaluates on the host, hence the same float
__device__ __forceinline__ float ema_decay_dev(float cap, const uint64_t* n_dev) {
    const double n = (double)*n_dev;
    return (float)fmin((double)cap, (1.0 + n) / (10.0 + n));
}
// VW floats per lane over n / VW lanes, then the n % VW elements behind them one per thread (G's 5 191 687 is odd: the tail is live)
template <int VW>
__global__ __launch_bounds__(256) void ema_k(float* __restrict__ e, const float* __restrict__ p, long n, float d, const uint64_t* n_dev) {
    if (n_dev) d = ema_decay_dev(d, n_dev);
    const float omd = 1.f - d;
    const long nv = n / VW;
    CG_GRID_STRIDE(i, nv) {
        const cg::Vec<VW> P = cg::Vec<VW>::load(p, i);
        cg::Vec<VW> E = cg::Vec<VW>::load(e, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) E[k] = ema_elem(E[k], P[k], d, omd);
        E.store(e, i);
    }
    if (VW > 1) {
        const long r = nv * VW + blockIdx.x * (long)blockDim.x + threadIdx.x;
        if (r < n) e[r] = ema_elem(e[r], p[r], d, omd);
    }
}
// penalty + clamp + Adam + the running average in one pass: p' never leaves the registers between the two
template <int VW>
__global__ __launch_bounds__(256) void adam_ema_k(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                  float* __restrict__ e, long n, float step, float b1, float b2, float eps, float l1,
                                                  float l2, float clampv, int write_back, float lr, const uint64_t* t_dev, float d,
                                                  const uint64_t* n_dev) {
    if (t_dev) step = adam_step_dev(lr, b1, b2, t_dev);
    if (n_dev) d = ema_decay_dev(d, n_dev);
    const float omd = 1.f - d;
    const long nv = n / VW;
    CG_GRID_STRIDE(i, nv) {
        cg::Vec<VW> P = cg::Vec<VW>::load(p, i), G = cg::Vec<VW>::load(g, i), M = cg::Vec<VW>::load(m, i), V = cg::Vec<VW>::load(v, i);
        cg::Vec<VW> E = cg::Vec<VW>::load(e, i);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            adam_elem(P[k], G[k], M[k], V[k], step, b1, b2, eps, l1, l2, clampv);
            E[k] = ema_elem(E[k], P[k], d, omd);
        }
        M.store(m, i); V.store(v, i); P.store(p, i); E.store(e, i);
        if (write_back) G.store(g, i);
    }
    if (VW > 1) {
        const long r = nv * VW + blockIdx.x * (long)blockDim.x + threadIdx.x;
        if (r < n) {
            float pi = p[r], gi = g[r], mi = m[r], vi = v[r];
            adam_elem(pi, gi, mi, vi, step, b1, b2, eps, l1, l2, clampv);
            m[r] = mi; v[r] = vi; p[r] = pi;
            e[r] = ema_elem(e[r], pi, d, omd);
            if (write_back) g[r] = gi;
        }
    }
}
__device__ __forceinline__ float pen_clamp(float pi, float gi, float l1, float l2, float clampv) {
    if (l1 != 0.f || l2 != 0.f) {
        const float sg = pi > 0.f ? 1.f : (pi < 0.f ? -1.f : 0.f);
        gi += sg * l1 + pi * l2;
    }
    if (clampv > 0.f) gi = fminf(fmaxf(gi, -clampv), clampv);
    return gi;
}
__global__ void sgd_k(float* p, float* g, float* v, long n, float lr, float mom, float damp, float l1, float l2,
                      float clampv, int write_back) {
    CG_GRID_STRIDE(i, n) {
        const float pi = p[i];
        const float gi = pen_clamp(pi, g[i], l1, l2, clampv);
        float d = gi;
        if (mom != 0.f) { d = mom * v[i] + (1.f - damp) * gi; v[i] = d; }
        p[i] = pi - lr * d;
        if (write_back) g[i] = gi;
    }
}
__global__ void adagrad_k(float* p, float* g, float* var, long n, float lr, float l1, float l2, float clampv,
                          int write_back) {
    CG_GRID_STRIDE(i, n) {
        const float pi = p[i];
        const float gi = pen_clamp(pi, g[i], l1, l2, clampv);
        const float vi = var[i] + gi * gi;
        var[i] = vi;
        p[i] = pi - lr * gi / (sqrtf(vi) + 1e-10f);
        if (write_back) g[i] = gi;
    }
}
// Adam's step size with the bias correction of step t >= 1, on the host
float adam_step_host(float lr, float beta1, float beta2, int t) {
    const double bc1 = 1.0 - pow((double)beta1, (double)t);
    const double bc2 = 1.0 - pow((double)beta2, (double)t);
    return (float)((double)lr * sqrt(bc2) / bc1);
}
}  // namespace

extern "C" {

int cg_adam_step(void* stream, float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                 float eps, int t, float l1, float l2, float clamp, int write_back_grad) {
    CG_REQUIRE(p && g && m && v && t >= 1, "cg_adam_step: bad args");
    CG_EW_LAUNCH(adam_k, n, p, g, m, v, n, adam_step_host(lr, beta1, beta2, t), beta1, beta2, eps, l1, l2, clamp, write_back_grad, lr, (const uint64_t*)nullptr);
    return 0;
}
int cg_adam_step_dev(void* stream, float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                     float eps, const uint64_t* t_dev, float l1, float l2, float clamp, int write_back_grad) {
    CG_REQUIRE(p && g && m && v && t_dev, "cg_adam_step_dev: bad args");
    CG_EW_LAUNCH(adam_k, n, p, g, m, v, n, 0.f, beta1, beta2, eps, l1, l2, clamp, write_back_grad, lr, t_dev);
    return 0;
}
#define EMA_DECAY_OK(d) ((d) > 0.f && (d) < 1.f)

int cg_ema_update(void* stream, float* e, const float* p, long n, float decay) {
    CG_REQUIRE(e && p, "cg_ema_update: null pointer");
    CG_REQUIRE(EMA_DECAY_OK(decay), "cg_ema_update: decay %g outside (0, 1)", (double)decay);
    CG_EW_LAUNCH_V(cg::vec_ok(0, e, p), ema_k<V>, n, e, p, n, decay, (const uint64_t*)nullptr);
    return 0;
}
int cg_ema_update_dev(void* stream, float* e, const float* p, long n, float decay_cap, const uint64_t* n_dev) {
    CG_REQUIRE(e && p && n_dev, "cg_ema_update_dev: null pointer");
    CG_REQUIRE(EMA_DECAY_OK(decay_cap), "cg_ema_update_dev: decay %g outside (0, 1)", (double)decay_cap);
    CG_EW_LAUNCH_V(cg::vec_ok(0, e, p), ema_k<V>, n, e, p, n, decay_cap, n_dev);
    return 0;
}
int cg_adam_step_ema(void* stream, float* p, float* g, float* m, float* v, float* e, long n, float lr, float beta1, float beta2,
                     float eps, int t, float l1, float l2, float clamp, int write_back_grad, float decay) {
    CG_REQUIRE(p && g && m && v && e, "cg_adam_step_ema: null pointer");
    CG_REQUIRE(t >= 1, "cg_adam_step_ema: step count t = %d < 1", t);
    CG_REQUIRE(EMA_DECAY_OK(decay), "cg_adam_step_ema: decay %g outside (0, 1)", (double)decay);
    CG_EW_LAUNCH_V(cg::vec_ok(0, p, g, m, v, e), adam_ema_k<V>, n, p, g, m, v, e, n, adam_step_host(lr, beta1, beta2, t), beta1, beta2, eps, l1, l2,
                   clamp, write_back_grad, lr, (const uint64_t*)nullptr, decay, (const uint64_t*)nullptr);
    return 0;
}
int cg_adam_step_ema_dev(void* stream, float* p, float* g, float* m, float* v, float* e, long n, float lr, float beta1, float beta2,
                         float eps, const uint64_t* t_dev, float l1, float l2, float clamp, int write_back_grad, float decay_cap,
                         const uint64_t* n_dev) {
    CG_REQUIRE(p && g && m && v && e && t_dev && n_dev, "cg_adam_step_ema_dev: null pointer");
    CG_REQUIRE(EMA_DECAY_OK(decay_cap), "cg_adam_step_ema_dev: decay %g outside (0, 1)", (double)decay_cap);
    CG_EW_LAUNCH_V(cg::vec_ok(0, p, g, m, v, e), adam_ema_k<V>, n, p, g, m, v, e, n, 0.f, beta1, beta2, eps, l1, l2, clamp, write_back_grad, lr,
                   t_dev, decay_cap, n_dev);
    return 0;
}
#undef EMA_DECAY_OK
int cg_sgd_step(void* stream, float* p, float* g, float* v, long n, float lr, float momentum, float dampening, float l1,
                float l2, float clamp, int write_back_grad) {
    CG_REQUIRE(p && g && (v || momentum == 0.f), "cg_sgd_step: bad args");
    CG_EW_LAUNCH(sgd_k, n, p, g, v, n, lr, momentum, dampening, l1, l2, clamp, write_back_grad);
    return 0;
}
int cg_adagrad_step(void* stream, float* p, float* g, float* var, long n, float lr, float l1, float l2, float clamp,
                    int write_back_grad) {
    CG_REQUIRE(p && g && var, "cg_adagrad_step: bad args");
    CG_EW_LAUNCH(adagrad_k, n, p, g, var, n, lr, l1, l2, clamp, write_back_grad);
    return 0;
}
}  // extern "C"
