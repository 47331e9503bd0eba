// net_plan.h - what a plan of the planned executor is made of (included by net.hip alone: one translation unit).
//
// The descriptors the compiler (net_compiler.h) fills and the runtime (net.hip) reads - Val, Mod, Geo, Seg, MS, Op, Prog, Net, Run -,
// the launch table generated from include/catgan.h (net_ktable.inc: the real entry points and their recording stubs) and the trace
// helpers the stubs write through.
#pragma once
#include <stdarg.h>

#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"

namespace {

using std::vector;

struct Net;
thread_local Net* g_cur_net = nullptr;   // the net whose ops are running (trace stubs resolve pointers through it)

struct TraceLine {
    std::string s;
    explicit TraceLine(const char* name) { s = "call|"; s += name; }
    void stream(void* st);
    void ptr(const void* p);
    void parr(const void* const* a, int n) {
        if (!a) { s += "|n"; return; }
        s += "|a:" + std::to_string(n) + ":";
        for (int i = 0; i < n; ++i) { if (i) s += ","; s += pname(a[i]); }
    }
    void iarr(const int* a, int n) {
        s += "|I:";
        for (int i = 0; a && i < n; ++i) { if (i) s += ","; s += std::to_string(a[i]); }
    }
    void i(long long v) { s += "|i:" + std::to_string(v); }
    void u(unsigned long long v) { s += "|u:" + std::to_string(v); }
    void f(double v) { char b[64]; snprintf(b, sizeof b, "|f:%a", v); s += b; }
    static std::string pname(const void* p);
    int done();
};

#include "net_ktable.inc"

// ------------------------------------------------------------------------------------------------ descriptors
enum Kind {
    K_SEQ = 0, K_CONCAT = 1, K_CONCATTABLE = 2, K_LINEAR = 3, K_CONV = 4, K_PRELU = 5, K_LRELU = 6, K_SIGMOID = 7, K_BN = 8,
    K_VIEW = 9, K_COPY = 10, K_TRANSPOSE = 11, K_UPS = 12, K_AVGPOOL = 13, K_MAXPOOL = 14, K_SDROP = 15, K_DROP = 16,
    K_AFFMAT = 17, K_AFFGRID = 18, K_SAMPLER = 19, K_COUNT
};
enum { PLAIN = 0, NHWC = 1 };
enum { EXT_NONE = 0, EXT_X = 1, EXT_GY = 2 };

// A tensor as the planner sees it: where it lives, its logical (Torch7) shape, its physical layout.
struct Val {
    float* p = nullptr;        // device address (ext == EXT_NONE)
    int ext = EXT_NONE;        // else: byte offset `off` from the caller's input (EXT_X) / gradOutput (EXT_GY) pointer
    size_t off = 0;
    int nd = 0;
    long d[4] = {0, 0, 0, 0};  // logical shape; fmt NHWC: [N,C,H,W] stored as [N,H>>ups,W>>ups,C]
    int fmt = PLAIN;
    int ups = 0;               // logical H,W are twice the physical ones (virtual nn.SpatialUpSamplingNearest(2))
    uint64_t blk = 0;          // this tensor is slice gi of gc equal slices of the block whose key is blk (0: not a slice)
    int gi = 0, gc = 0;
    bool is_tab = false;       // nn.ConcatTable output: a table of tensors
    vector<Val> tab;
    bool none = true;

    long numel() const { long n = 1; for (int i = 0; i < nd; ++i) n *= d[i]; return n; }
    long phys() const { return numel() >> (2 * ups); }
    uint64_t key() const { return ext ? (((uint64_t)ext << 60) | (uint64_t)off) : (uint64_t)(uintptr_t)p; }
    bool same_shape(const Val& o) const {
        if (nd != o.nd) return false;
        for (int i = 0; i < nd; ++i) if (d[i] != o.d[i]) return false;
        return true;
    }
    Val at(size_t byte_off) const {   // same descriptor, address moved
        Val v = *this;
        if (ext) v.off += byte_off; else v.p = (float*)((char*)p + byte_off);
        return v;
    }
};

Val mkval(float* p, std::initializer_list<long> dims, int fmt = PLAIN, int ups = 0) {
    Val v; v.p = p; v.nd = (int)dims.size(); int i = 0; for (long x : dims) v.d[i++] = x; v.fmt = fmt; v.ups = ups; v.none = false;
    return v;
}
Val reshape(const Val& x, std::initializer_list<long> dims, int fmt, int ups = 0, bool keep_grp = false) {
    Val v = x; v.nd = (int)dims.size(); int i = 0; for (long q : dims) v.d[i++] = q; for (; i < 4; ++i) v.d[i] = 0;
    v.fmt = fmt; v.ups = ups;
    if (!keep_grp) { v.blk = 0; v.gi = v.gc = 0; }
    return v;
}

struct Mod {
    int id = 0, kind = 0, parent = -1;
    vector<int> kids;
    long ia[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float fa[4] = {0, 0, 0, 0};
    int train = 1;
    float *w = nullptr, *gw = nullptr, *b = nullptr, *gb = nullptr, *rmean = nullptr, *rvar = nullptr;
    // kernel-side copies of a conv / linear layer's weight (shared by every compiled plan of the net)
    float *wf = nullptr, *wb = nullptr;          // plain: wf[(tap*Cin+ci)][Cout], wb (flipped taps) or NULL for 1x1
    int pk_map = -1;                             // 0 plain / 1 map (cg_pack_conv_weight_map) layout currently allocated; -1 none
    long map_c = 0, map_h = 0, map_w = 0;
    bool dirty_plain = true;
    float *wf_ph = nullptr, *wb_ph = nullptr;    // behind a folded 2x upsampling: phase-summed
    float *u_fwd = nullptr, *u_bwd = nullptr;    // Winograd-domain phase kernels
    float *u22 = nullptr, *u22b = nullptr;       // F(2x2,2x2) forward / data-gradient kernels of a 3x3 layer behind a folded upsampling
    bool wino = false, dirty_ups = true;
    bool is_gemm() const { return kind == K_LINEAR || kind == K_CONV; }
    bool is_act() const { return kind == K_PRELU || kind == K_LRELU; }
    bool is_pool() const { return kind == K_AVGPOOL || kind == K_MAXPOOL; }
    bool is_container() const { return kind <= K_CONCATTABLE; }
    long Cin() const { return kind == K_LINEAR ? ia[0] : ia[0]; }
    long Cout() const { return ia[1]; }
    long kW() const { return kind == K_CONV ? ia[2] : 1; }
    long kH() const { return kind == K_CONV ? ia[3] : 1; }
    long padW() const { return kind == K_CONV ? ia[4] : 0; }
    long padH() const { return kind == K_CONV ? ia[5] : 0; }
};

struct Geo {   // the 10 geometry arguments of the convolution entry points
    int N, Hp, Wp, Cin, Cout, kH, kW, padH, padW, ups;
    bool operator==(const Geo& o) const {
        return N == o.N && Hp == o.Hp && Wp == o.Wp && Cin == o.Cin && Cout == o.Cout && kH == o.kH && kW == o.kW && padH == o.padH &&
               padW == o.padW && ups == o.ups;
    }
};
#define GEO(g) (g).N, (g).Hp, (g).Wp, (g).Cin, (g).Cout, (g).kH, (g).kW, (g).padH, (g).padW, (g).ups

struct Seg { int kind; int i, j; };   // kinds below; modules [i, j) of a Sequential
enum { S_ONE = 0, S_GEMM_ACT, S_ACT_POOL, S_VIEW_GEMM, S_VIEW_GEMM_ACT, S_GEMM_BN_ACT, S_CAT_DROP, S_HEAD };

// What a module left behind in one compiled plan (the attributes the Python twin kept on the module objects).
struct MS {
    Val x, out, gin;             // input as consumed, output, gradInput
    Val p;                       // AffineTransformMatrixGenerator: its parameter input
    Val noise, noise_block;      // dropout masks
    Val in_img, in_grid;         // sampler inputs
    uint64_t stk = 0;            // key of the block a stacked forward produced (first sibling only)
    bool shared_in = false;      // pooling: siblings shared one launch
    bool has_shared = false; Val shared_out, shared_grids;   // sampler: shared-image launch
    bool skip = false;           // nn.View fused into the linear layer behind it
    long in_shape[4] = {0, 0, 0, 0}; int in_nd = 0;
    bool map_in = false; long mc = 0, mh = 0, mw = 0;        // nn.Linear consuming an NHWC map
    bool use_wino = false, use_wino22 = false;
    bool fused = false; int fG = 0; Val fX, fmask; long fN = 0, fC = 0, fH = 0, fW = 0;   // act_pool segment state (on the activation)
    bool bn_fused = false; long bnM = 0, bnC = 0;            // gemm_bn_act segment state (on the batch-norm)
    double count = 0;            // BN: samples behind the statistics (x world under sync-BN)
    vector<long> sizes;          // nn.Concat: channels per branch
    vector<Seg> ran;             // nn.Sequential: the plan its forward ran
    bool ran_set = false;
    void* wg_ws = nullptr; size_t wg_ws_bytes = 0; bool wg_pending = false;   // deferred weight-gradient workspace
    bool loc_fused = false; int locG = 0; long locN = 0;                      // [locnet, AffMat, AffGrid] ran as cg_locnet_forward
    bool cat_drop = false;                                                   // nn.Concat: the SpatialDropout behind it ran inside its launch
    bool head_fused = false; Val hz;                                         // nn.Dropout: [Dropout, Linear, Sigmoid] ran as one launch (hz = the linear output)
    void* loc_ws[4] = {nullptr, nullptr, nullptr, nullptr}; size_t loc_ws_bytes[4] = {0, 0, 0, 0};
    std::map<std::string, Val> bufs;
};

struct Run;
struct Op { int sidx; std::function<int(Run&)> fn; };

struct Prog {
    Net* net = nullptr;
    Val in;                                    // input descriptor the plan was compiled for (ext = EXT_X)
    std::map<int, MS> ms;
    vector<Op> fwd;
    vector<Op> bwd[2];                         // [0] updateGradInput only, [1] backward (gradInput + accGradParameters)
    bool have_bwd[2] = {false, false};
    Val out, gin[2];
    long draws = 0;                            // counter-stream draws of one forward
    int nstreams = 1;                          // 1 + side streams this plan uses
    vector<void*> ws; vector<size_t> ws_bytes; // split-K scratch per stream index (grow-only)
    unsigned long opt_epoch = 0;
    vector<std::pair<float*, long>> buckets;   // gradient buckets of the root Sequential (first module index order)
    vector<int> bucket_first;
    std::map<int, int> ups_first_op;           // module id of a layer behind a folded upsampling -> index of its first forward op
    struct BnRun { Mod* bn; Val sums; double cnt; long C; float mom; };
    vector<BnRun> bn_runs;                     // training-mode batch-norms of the forward pass (cg_net_apply_running)
    bool running_pending = false;
};

typedef void* (*alloc_fn_t)(void* user, size_t bytes);
typedef int (*hook_fn_t)(void* user, int what, void* buf, size_t count, int dtype, void* stream);

struct Region { const char* base; size_t bytes; };

struct Net {
    vector<std::unique_ptr<Mod>> mods;
    std::map<std::string, std::unique_ptr<Prog>> progs;
    Prog* last = nullptr;                      // plan of the most recent forward (what backward continues)
    vector<hipStream_t> side; vector<hipEvent_t> side_ev; hipEvent_t fork_ev = nullptr;
    hipEvent_t pack_fork_ev = nullptr, pack_ev = nullptr;   // weight re-packing beside the head of the forward pass (sync_packs)
    hipEvent_t wg_fork_ev[4] = {nullptr, nullptr, nullptr, nullptr}, wg_join_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // weight-gradient streams (option wgrad_stream)
    alloc_fn_t alloc_fn = nullptr; void* alloc_user = nullptr;
    hook_fn_t hook = nullptr; void* hook_user = nullptr;
    void *comm_bn = nullptr, *comm_grad = nullptr; int world = 1; int sync_bn = 1; int bucket_overlap = 0;
    int hook_too = 0;                          // communicator collective AND host hook (cg_net_set_dp bucket_overlap & 2)
    vector<void*> owned;
    vector<Region> regions;
    bool params_dirty = true;
    int qmap[8] = {-1, 0, 0, 0, 0, 0, 0, 0};  // hardware-queue class of stream index t (ensure_streams)
    bool pack_inflight = false;               // sync_packs forked a re-packing that a LATER pass on another stream may still have to wait for
    int defer_running = 0;                     // run-time switch: batch-norm forwards leave the running statistics to cg_net_apply_running
    // cg_net_forward_pair: the second pass's stream (another hardware queue than the caller's), fork / "first pass complete" / join events
    hipStream_t pair_stream = nullptr; hipEvent_t pair_fork_ev = nullptr, pair_a_ev = nullptr, pair_join_ev = nullptr;
    bool pair_pending = false; float* pair_y = nullptr; Val pair_out;   // pass 2's output: where it is, its descriptor
    bool fresh_allocs = false;                 // library-owned buffers were allocated + zeroed since the last device synchronise
    // options
    int trace = 0, overlap_groups = 1, defer_wgrad = 1, winograd = 1, share_pool = 1, sampler_shared = 1, view_fuse = 1,
        cat_fuse = 1, stacking = 1, grouped = 1, fusion = 1, fuse_locnet = 1, pack_overlap = 1, head_fuse = 1, wgrad_stream = 1,
        wino_dsplit = 1;       // the F(2x2,3x3) data gradient in K slices when its unsplit launch is <= one workgroup per CU (cg_conv2d_ups2_wino_dgrad_split)
    long wino_min_tiles = 2048;
    int wino22 = 3;                            // F(2x2,2x2) for upsample2 -> conv3x3 above wino_min_tiles: bit 0 forward, 1 data gradient
                                               // (option "winograd22"; the weight gradient is 292 -> 257 us alone but no gain in the step: off)
    std::string trace_log;
    const KTable* K = &kRealTable;
    vector<void*> trace_streams;               // stream handle -> index in trace mode
    char err[512] = {0};
};

struct Run {
    Net* net; Prog* pr;
    hipStream_t st[8];                          // [0] the caller's, [1..3] side streams of branch groups, [4 + s] the weight-gradient stream beside stream s
    const float* x = nullptr; const float* gy = nullptr;
    uint64_t seed = 0, roff = 0; const uint64_t* rbase = nullptr;
    float scale = 1.f;
    int cur = 0;                                // stream index of the op being issued
    void* S(int sidx) const { return (void*)st[sidx]; }
    void* CS() const { return (void*)st[cur]; }
    float* P(const Val& v) const {
        if (v.none) return nullptr;
        if (v.ext == EXT_X) return (float*)((char*)x + v.off);
        if (v.ext == EXT_GY) return (float*)((char*)gy + v.off);
        return v.p;
    }
    void* W() const { return pr->ws[cur]; }
    size_t WB() const { return pr->ws_bytes[cur]; }
};

// ------------------------------------------------------------------------------------------------ tracing
std::string TraceLine::pname(const void* p) {
    if (!p) return "n";
    Net* n = g_cur_net;
    if (n)
        for (size_t k = 0; k < n->regions.size(); ++k) {
            const Region& r = n->regions[k];
            if ((const char*)p >= r.base && (const char*)p < r.base + r.bytes)
                return "r" + std::to_string(k) + "+" + std::to_string((const char*)p - r.base);
        }
    char b[40]; snprintf(b, sizeof b, "?%p", p);
    return b;
}
void TraceLine::ptr(const void* p) { s += "|"; s += pname(p); }
void TraceLine::stream(void* st) {
    Net* n = g_cur_net;
    int k = -1;
    if (n) for (size_t i = 0; i < n->trace_streams.size(); ++i) if (n->trace_streams[i] == st) k = (int)i;
    s += "|s" + std::to_string(k);
}
int TraceLine::done() {
    if (g_cur_net) { g_cur_net->trace_log += s; g_cur_net->trace_log += "\n"; }
    return 0;
}
void trace_note(Net* n, const std::string& s) { if (n->trace) { n->trace_log += s; n->trace_log += "\n"; } }

}  // namespace
