// The finish of a weight gradient: the split partial sums that a weight-gradient launch (igemm_tn / igemm_tng of gemm.hip, the skinny
// kernels of skinny.hip) left in its workspace, reduced into Torch7's canonical gradWeight / gradBias, accumulate semantics:
//   plain: gw[co][ci][tap] += scale * sum_s part[s][tap*Cin+ci][co]
//   UPS  : gw[co][ci][dy][dx] += scale * sum_s sum_{a,b} part[s][2a+b][(map(a,dy)*kp + map(b,dx))*Cin + ci][co]
//   bias : gb[co] += scale * sum_{s,p} bias_part[s][p][co]
// cg::wgrad_finish (common.h) is the one way in.  Two orders of addition exist, and every form below keeps one of them:
//   tiled and transpose forms: splits in ascending order, the phases 0..3 inside each split;
//   small forms: lane group ln = tid / 32 adds splits ln, ln + 8, ... (again the phases inside a split), then groups 0..7 are added in order.
// Which geometry gets which form is decided in cg::wgrad_finish and red_job and nowhere else.
#include "common.h"
#include <mutex>
#include <unordered_map>
#include <vector>

namespace {

using cg::f4c;
using cg::ld4;
using cg::phase_map;
using cg::sel4;

// ---- the additions, each written once ---------------------------------------------------------------------------------------------
// One canonical element (tap, ci, co) of a group's partials pg: splits sp0, sp0 + STEP, ... in order and, behind an upsampling, the four
// phases inside each split (phase p holds the element at its low-res tap tp).  plane: floats of a phase.
template <bool UPS, int STEP>
__device__ __forceinline__ float fold(const float* pg, int tap, int ci, int co, int Cin, int Cout, int k, int pad, int kp, long plane, int S,
                                      long sstride, int sp0) {
    float s = 0.f;
    if (UPS) {
        const int dy = tap / k, dx = tap - dy * k;
        for (int sp = sp0; sp < S; sp += STEP)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int tp = phase_map(p >> 1, dy, pad) * kp + phase_map(p & 1, dx, pad);
                s += pg[(long)sp * sstride + (long)p * plane + ((long)tp * Cin + ci) * Cout + co];
            }
    } else {
        const long o = ((long)tap * Cin + ci) * Cout + co;
        constexpr int kInFlight = STEP == 8 ? 4 : 1;   // the small forms keep four splits in flight; unrolled, the tiled launches measured slower
#pragma unroll kInFlight
        for (int sp = sp0; sp < S; sp += STEP) s += pg[(long)sp * sstride + o];
    }
    return s;
}

__device__ __forceinline__ void add4(float4& s, const float4& p) { s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w; }
// the same for four consecutive elements at src (16-byte aligned, plain layout): planes sp0, sp0 + STEP, ... in order, four in flight
template <int STEP>
__device__ __forceinline__ float4 fold4(const float* src, int S, long sstride, int sp0) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int sp = sp0;
    for (; sp + 3 * STEP < S; sp += 4 * STEP) {
        const float4 p0 = ld4(src + (long)sp * sstride), p1 = ld4(src + (long)(sp + STEP) * sstride);
        const float4 p2 = ld4(src + (long)(sp + 2 * STEP) * sstride), p3 = ld4(src + (long)(sp + 3 * STEP) * sstride);
        add4(s, p0); add4(s, p1); add4(s, p2); add4(s, p3);
    }
    for (; sp < S; sp += STEP) add4(s, ld4(src + (long)sp * sstride));
    return s;
}

// second half of the small order: the sums of the eight lane groups, in order
__device__ __forceinline__ float lane_groups_sum(float (*sh)[33], int ol) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) t += sh[r][ol];
    return t;
}

// gb[c] += scale * sum_{s,p} bp[s * bsstride + p * Cout + c] for the 32 channels from c0 (S splits x P phases of one group, the small
// order over the S * P entries): the stand-alone kernel's body and the bias blocks of the small and batch kernels
__device__ __forceinline__ void bias_sum_block(float (*sh)[33], const float* bp, float* gb, int c0, int S, int P, long bsstride, int Cout, float scale) {
    const int cl = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int c = c0 + cl;
    float s = 0.f;
    if (c < Cout)
        for (int i = ln; i < S * P; i += 8) s += bp[(long)(i / P) * bsstride + (long)(i % P) * Cout + c];
    sh[ln][cl] = s;
    __syncthreads();
    if (ln == 0 && c < Cout) gb[c] += scale * lane_groups_sum(sh, cl);
}

// ---- the tiled form ----------------------------------------------------------------------------------------------------------------
// One workgroup owns CI_T input channels x 32 output channels x all taps: reads are coalesced along co, the sums are transposed through
// LDS, writes are contiguous runs of CI_T*KK floats per co.  (A thread re-reads a phase's partial element once per canonical tap that
// folds onto it - 36 loads for 16 values of a 3x3 kernel behind an upsampling; a form that reads each once in 16-byte loads is open
// work)
template <bool UPS>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* part, float* gw, int Cin, int Cout, int k, int KK,
                                                           int pad, int kp, int S, float scale, int CI_T, long sstride) {
    extern __shared__ float sh[];  // [CI_T][KK][33]
    const int ci0 = blockIdx.x * CI_T, co0 = blockIdx.y * 32;
    const long plane = (long)(UPS ? kp * kp : KK) * Cin * Cout;
    const int n1 = KK * CI_T * 32;
    for (int idx = threadIdx.x; idx < n1; idx += 256) {
        const int co_l = idx & 31;
        const int r = idx >> 5;
        const int ci_l = r % CI_T, tap = r / CI_T;
        const int ci = ci0 + ci_l, co = co0 + co_l;
        float s = 0.f;
        if (ci < Cin && co < Cout) s = fold<UPS, 1>(part, tap, ci, co, Cin, Cout, k, pad, kp, plane, S, sstride, 0);
        sh[(ci_l * KK + tap) * 33 + co_l] = s;   // row = position in the output run: the transposed read below walks rows with stride 33 (odd: conflict-free)
    }
    __syncthreads();
    const int run = CI_T * KK;
    for (int idx = threadIdx.x; idx < n1; idx += 256) {
        const int j = idx % run, co_l = idx / run;
        const int ci_l = j / KK, tap = j - ci_l * KK;
        const int ci = ci0 + ci_l, co = co0 + co_l;
        if (ci < Cin && co < Cout) {
            float* dst = gw + ((long)co * Cin + ci) * KK + tap;
            *dst += scale * sh[j * 33 + co_l];
        }
    }
}

// gb[c] += scale * sum_{s,p} bias_part[s*P+p][c]; 32 channels x 8 partial-sum lanes per workgroup
__global__ __launch_bounds__(256) void bias_part_reduce_kernel(const float* bp, float* gb, int S, int P, long sstride, int Cout, float scale) {
    __shared__ float sh[8][33];
    bias_sum_block(sh, bp, gb, blockIdx.x * 32, S, P, sstride, Cout, scale);
}

// ---- the small forms: one job = one layer's partials, all groups of a grouped launch and their bias gradients ---------------------------
// For weight tensors where the tiled form would not fill the chip.  A job is ngroups x (wblocks weight blocks + bblocks bias blocks of 32
// channels); what a weight block is depends on the job (tr / v4 / neither, below).
struct RedPtrs { float* gw0; float* gw1; float* gw2; float* gw3; float* gb0; float* gb1; float* gb2; float* gb3;
                 long gws; };   // gws != 0: group g accumulates into gw0 + g * gws (strided groups, no bias gradients)
struct RedJob {
    const float* part; const float* bias_part;
    RedPtrs rp;
    long sstride, gstride, bsstride;   // floats between consecutive splits / groups of part, between consecutive splits of bias_part
    int Cin, Cout, k, KK, pad, kp, S, P, ups, ngroups, wblocks, bblocks;
    int block0;  // cg_conv2d_wgrad_flush: the job's first workgroup in the batch launch
    float scale;
    int tr;      // KK == 1, planes multiples of 32: the weight blocks are 32 x 32 transpose tiles (wgrad_reduce_t_tile), not 32-element runs
    int v4;      // plain layout, Cout % 4 == 0, 16-byte aligned planes: the weight blocks are 128-element runs (wgrad_reduce_small_v4)
};
constexpr int kRedJobs = 20;
struct RedJobTable { RedJob j[kRedJobs]; int n; };

__device__ __forceinline__ float* gw_of(const RedPtrs& rp, int group) {
    return rp.gws ? rp.gw0 + (long)group * rp.gws : sel4(group, rp.gw0, rp.gw1, rp.gw2, rp.gw3);
}

// a workgroup owns 32 consecutive partial elements and splits the S partials over 8 lane groups
template <bool UPS>
__device__ __forceinline__ void wgrad_reduce_small(float (*sh)[33], const RedJob& J, int group, int bx) {
    const int ol = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const long total = (long)J.KK * J.Cin * J.Cout, plane = (long)(UPS ? J.kp * J.kp : J.KK) * J.Cin * J.Cout;
    const long i = bx * 32L + ol;
    int co = 0, ci = 0, tap = 0;
    float s = 0.f;
    if (i < total) {
        co = (int)(i % J.Cout);
        const long r = i / J.Cout;
        ci = (int)(r % J.Cin);
        tap = (int)(r / J.Cin);
        s = fold<UPS, 8>(J.part + (long)group * J.gstride, tap, ci, co, J.Cin, J.Cout, J.k, J.pad, J.kp, plane, J.S, J.sstride, ln);
    }
    sh[ln][ol] = s;
    __syncthreads();
    if (ln == 0 && i < total) gw_of(J.rp, group)[((long)co * J.Cin + ci) * J.KK + tap] += J.scale * lane_groups_sum(sh, ol);
}

// The plain (not phase-folded) weight blocks with 16-byte loads (round 5): a workgroup owns 128 consecutive partial elements - lane ol
// the float4 at bx * 128 + 4 ol, the S partial planes split over the 8 lane groups as above, four planes in flight per thread - and
// 128 threads add the eight lane sums in the same order and scatter them to the canonical layout.  Same bits as the 32-element form;
// a quarter of the workgroups and load instructions.
__device__ __forceinline__ void wgrad_reduce_small_v4(float* shf, const RedJob& J, int group, int bx) {
    float4* sh4 = reinterpret_cast<float4*>(shf);     // [8][32]
    const int ol = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const long total = (long)J.KK * J.Cin * J.Cout;
    const long i = bx * 128L + 4 * ol;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < total) s = fold4<8>(J.part + (long)group * J.gstride + i, J.S, J.sstride, ln);
    sh4[ln * 32 + ol] = s;
    __syncthreads();
    if (ln < 4 && i < total) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) t += f4c(sh4[r * 32 + ol], ln);
        const long e = i + ln;                      // element (tap, ci, co) of the partial plane
        const int co = (int)(e % J.Cout);
        const long rr = e / J.Cout;
        const int ci = (int)(rr % J.Cin), tap = (int)(rr / J.Cin);
        gw_of(J.rp, group)[((long)co * J.Cin + ci) * J.KK + tap] += J.scale * t;
    }
}

// KK == 1 (linear layers, the Winograd-domain products of winograd.hip): canonical gw[co][ci] += scale * sum_s part[s][ci][co] is a
// TRANSPOSE of the partial planes.  The forms above give a workgroup 32 consecutive partial elements and scatter them to
// addresses Cin floats apart: 65 536 workgroups of 1 KB for the 16 Winograd products - 69 us alone, 295 us beside the data-gradient
// chain (profiles/r04_eager_breakdown.txt).  Here: 32 x 32 tiles through LDS, 128-byte rows both ways, splits added in order.
__device__ __forceinline__ void wgrad_reduce_t_tile(float (*t)[33], const float* __restrict__ pg, float* __restrict__ gw, int ci0, int co0,
                                                    int Cin, int Cout, int S, long sstride, float scale) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if ((Cout & 3) == 0 && (sstride & 3) == 0 && ((uintptr_t)pg & 15) == 0) {
        // 16-byte loads (round 5): thread = (row r = tid / 8, four columns)
        const int r = threadIdx.x >> 3, c4 = threadIdx.x & 7;
        const float4 s = fold4<1>(pg + (long)(ci0 + r) * Cout + co0 + 4 * c4, S, sstride, 0);
        t[r][4 * c4] = s.x; t[r][4 * c4 + 1] = s.y; t[r][4 * c4 + 2] = s.z; t[r][4 * c4 + 3] = s.w;
    } else
#pragma unroll
    for (int r = ty; r < 32; r += 8) t[r][tx] = fold<false, 1>(pg, 0, ci0 + r, co0 + tx, Cin, Cout, 1, 0, 0, 0, S, sstride, 0);
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) gw[(long)(co0 + r) * Cin + ci0 + tx] += scale * t[tx][r];
}
__global__ __launch_bounds__(256) void wgrad_reduce_t_kernel(const float* __restrict__ part, float* __restrict__ gw0, long gws, int Cin,
                                                             int Cout, int S, long sstride, long gstride, float scale) {
    __shared__ float t[32][33];
    const int group = blockIdx.z;
    wgrad_reduce_t_tile(t, part + (long)group * gstride, gw0 + (long)group * gws, blockIdx.x * 32, blockIdx.y * 32, Cin, Cout, S, sstride, scale);
}

// block bx of group `group` of a job
__device__ __forceinline__ void red_block(float (*sh)[33], const RedJob& J, int group, int bx) {
    if (bx >= J.wblocks) {
        float* gb = sel4(group, J.rp.gb0, J.rp.gb1, J.rp.gb2, J.rp.gb3);
        if (gb) bias_sum_block(sh, J.bias_part + (long)group * J.P * J.Cout, gb, (bx - J.wblocks) * 32, J.S, J.P, J.bsstride, J.Cout, J.scale);
    } else if (J.tr) {
        const int nci = J.Cin / 32;
        wgrad_reduce_t_tile(sh, J.part + (long)group * J.gstride, gw_of(J.rp, group), (bx % nci) * 32, (bx / nci) * 32, J.Cin, J.Cout, J.S, J.sstride, J.scale);
    } else if (J.v4)
        wgrad_reduce_small_v4(&sh[0][0], J, group, bx);
    else if (J.ups)
        wgrad_reduce_small<true>(sh, J, group, bx);
    else
        wgrad_reduce_small<false>(sh, J, group, bx);
}

// one job: grid (wblocks + bblocks, ngroups).  One workgroup per block: a block is a short dependent chain (strided partial loads -> LDS ->
// one add), so a workgroup that walked several would serialise latency (round 4, same box: 6.32 / 6.38 / 6.40 ms per step at 0 / 8 / 32
// workgroups per CU) - unlike the grid-stride element-wise kernels (cg::ew_grid)
__global__ __launch_bounds__(256) void wgrad_reduce_small_kernel(RedJob J) {
    __shared__ __attribute__((aligned(16))) float sh[32][33];
    red_block(sh, J, (int)blockIdx.y, (int)blockIdx.x);
}

// SEVERAL layers in one launch (cg_conv2d_wgrad_flush): the deferred form of cg_conv2d_wgrad* runs only its GEMM and queues one RedJob;
// a dozen ~10 us reductions, each a short dependent chain, then overlap instead of queueing up behind one another.  Workgroup b belongs
// to the job whose [block0, block0 + ngroups * (wblocks + bblocks)) holds b.
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(RedJobTable t) {
    __shared__ __attribute__((aligned(16))) float sh[32][33];
    const int b = (int)blockIdx.x;
    int ji = 0;
    for (int q = 1; q < t.n; ++q)
        if (b >= t.j[q].block0) ji = q;
    const RedJob& J = t.j[ji];
    const int per = J.wblocks + J.bblocks;
    const int group = (b - J.block0) / per;
    red_block(sh, J, group, (b - J.block0) - group * per);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// reductions queued by the deferred entry points, per stream (one host thread per stream, but several streams may queue)
std::mutex g_red_mu;
std::unordered_map<hipStream_t, std::vector<RedJob>> g_red_queue;

// KK == 1, no phases, both plane counts multiples of 32: the finish is a transpose of 32 x 32 tiles
bool transposable(const cg::WgradParts& w) { return w.kH * w.kW == 1 && !w.ups && w.Cin % 32 == 0 && w.Cout % 32 == 0; }

RedJob red_job(const cg::WgradParts& w, bool defer) {
    RedJob job;
    memset(&job, 0, sizeof(job));
    const int nptr = w.gws ? 1 : w.ngroups;
    cg::set4(job.rp.gw0, job.rp.gw1, job.rp.gw2, job.rp.gw3, w.gw, nptr);
    cg::set4(job.rp.gb0, job.rp.gb1, job.rp.gb2, job.rp.gb3, w.gb, nptr);
    job.rp.gws = w.gws;
    job.part = w.part; job.bias_part = w.bias_part;
    job.Cin = w.Cin; job.Cout = w.Cout; job.k = w.kH; job.KK = w.kH * w.kW; job.pad = w.pad; job.ups = w.ups ? 1 : 0;
    job.kp = w.ups ? cg::phase_kp(w.kH, w.pad) : 0;
    job.S = w.S; job.P = w.ups ? 4 : 1; job.ngroups = w.ngroups; job.scale = w.scale;
    const long relems = (long)job.KK * w.Cin * w.Cout;                                  // canonical elements of a group
    job.gstride = (w.ups ? 4L * job.kp * job.kp : job.KK) * w.Cin * w.Cout;             // the P phase planes of a group
    job.sstride = w.ngroups * job.gstride;
    job.bsstride = (long)w.ngroups * job.P * w.Cout;
    job.wblocks = cg::cdiv(relems, 32); job.bblocks = w.bias_part ? cg::cdiv(w.Cout, 32) : 0;
    // a queued KK == 1 job (nn.Linear; D's 20480 -> 256 head is 5.2 M elements = 164 000 32-element blocks) reduces as transpose tiles
    if (defer && transposable(w)) {
        job.tr = 1; job.wblocks = (w.Cin / 32) * (w.Cout / 32);
    } else if (!w.ups && w.Cout % 4 == 0 && cg::al16(w.part) && job.sstride % 4 == 0 && job.gstride % 4 == 0) {
        job.v4 = 1; job.wblocks = cg::cdiv(relems, 128);
    }
    return job;
}

int small_reduce(hipStream_t st, bool defer, const RedJob& job) {
    if (defer) {
        std::lock_guard<std::mutex> lk(g_red_mu);
        g_red_queue[st].push_back(job);
        return 0;
    }
    hipLaunchKernelGGL(wgrad_reduce_small_kernel, dim3(job.wblocks + job.bblocks, job.ngroups), dim3(256), 0, st, job);
    CG_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int cg::wgrad_finish(hipStream_t st, const WgradParts& w, bool defer) {
    const RedJob job = red_job(w, defer);
    const int Cin = w.Cin, Cout = w.Cout, KK = job.KK;
    if (w.gws && transposable(w) && !w.bias_part) {
        hipLaunchKernelGGL(wgrad_reduce_t_kernel, dim3(Cin / 32, Cout / 32, w.ngroups), dim3(256), 0, st, w.part, w.gw[0], w.gws, Cin, Cout, w.S,
                           job.sstride, job.gstride, w.scale);
        CG_LAUNCH_CHECK();
        return 0;
    }
    // the tiled form's blocks: 8 input channels (64 of a KK == 1 layer), fewer while a block's sums exceed the LDS
    int ci_t = KK == 1 ? 64 : 8;
    while (ci_t > 1 && (size_t)KK * ci_t * 33 * sizeof(float) > 60000) ci_t >>= 1;
    const size_t shb = (size_t)KK * ci_t * 33 * sizeof(float);
    const dim3 rgrid(cg::cdiv(Cin, ci_t), cg::cdiv(Cout, 32));
    if ((long)rgrid.x * rgrid.y < cg::kNumCU) return small_reduce(st, defer, job);
    for (int gi = 0; gi < w.ngroups; ++gi) {
        const float* pg = w.part + gi * job.gstride;
        float* gwi = w.gws ? w.gw[0] + gi * w.gws : w.gw[gi];
        hipLaunchKernelGGL(w.ups ? wgrad_reduce_kernel<true> : wgrad_reduce_kernel<false>, rgrid, dim3(256), shb, st, pg, gwi, Cin, Cout, w.kH, KK,
                           w.pad, job.kp, w.S, w.scale, ci_t, job.sstride);
        CG_LAUNCH_CHECK();
        if (w.gb && w.gb[gi]) {
            hipLaunchKernelGGL(bias_part_reduce_kernel, dim3(cg::cdiv(Cout, 32)), dim3(256), 0, st, w.bias_part + (long)gi * job.P * Cout, w.gb[gi],
                               w.S, job.P, job.bsstride, Cout, w.scale);
            CG_LAUNCH_CHECK();
        }
    }
    return 0;
}

void cg::wgrad_discard_all() {
    std::lock_guard<std::mutex> lk(g_red_mu);
    for (auto& kv : g_red_queue) kv.second.clear();
}

extern "C" {

int cg_conv2d_wgrad_pending(void* stream, int* njobs) {
    CG_REQUIRE(njobs, "cg_conv2d_wgrad_pending: null pointer");
    std::lock_guard<std::mutex> lk(g_red_mu);
    auto it = g_red_queue.find(cg::S(stream));
    *njobs = it == g_red_queue.end() ? 0 : (int)it->second.size();
    return 0;
}

int cg_conv2d_wgrad_flush(void* stream) {
    hipStream_t st = cg::S(stream);
    std::vector<RedJob> jobs;
    {
        std::lock_guard<std::mutex> lk(g_red_mu);
        auto it = g_red_queue.find(st);
        if (it == g_red_queue.end() || it->second.empty()) return 0;
        jobs.swap(it->second);
    }
    for (size_t j0 = 0; j0 < jobs.size(); j0 += kRedJobs) {
        RedJobTable t;
        memset(&t, 0, sizeof(t));
        t.n = (int)std::min<size_t>(kRedJobs, jobs.size() - j0);
        int blocks = 0;
        for (int q = 0; q < t.n; ++q) {
            t.j[q] = jobs[j0 + q];
            t.j[q].block0 = blocks;
            blocks += t.j[q].ngroups * (t.j[q].wblocks + t.j[q].bblocks);
        }
        hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(blocks), dim3(256), 0, st, t);
        CG_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
