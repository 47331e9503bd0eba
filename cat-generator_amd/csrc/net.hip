// net.hip - the planned executor behind the C ABI (cg_net_*, cg_graph_*; include/catgan.h).
//
// A host (the LuaJIT layer, the Python twin, a C++ driver) describes a network module by module - the constructor calls of
// models.lua:138-160,196-228,640-711,814-906 map one to one onto cg_net_add - binds the parameter tensors its
// getParameters() produced (train.lua:184-185) and then calls cg_net_forward / cg_net_backward where the reference calls
// MODEL_X:forward / :backward / :updateGradInput (adversarial.lua:84-89,182-197).  Everything between those calls lives here:
//
//   * the plan: nn.Sequential's module list is cut into segments that run as fused launches (conv|linear -> activation in the GEMM
//     epilogue; activation -> 2x2 pooling -> spatial dropout in one pass; conv -> batch-norm (training) -> PReLU with the statistics
//     in the GEMM epilogue; nn.View -> nn.Linear reading the NHWC map directly);
//   * lockstep execution of structurally identical nn.Concat branches (D32_st3's three transformer branches, models.lua:653-678):
//     grouped GEMM launches, parameter-free layers as ONE launch over the stacked batch, shared pooling / shared-image sampling;
//   * the second group of branches on a side HIP stream (event fork / join), deferred + batched weight-gradient reductions,
//     one batched weight re-pack per parameter update, sync-BN / gradient-bucket collectives at their places in the sequence;
//   * buffers: every activation, gradient, mask and workspace is allocated when a (network, input shape) pair is first compiled,
//     so a compiled plan launches without allocating - which is what lets cg_graph_begin / _end capture a whole training
//     iteration of host code into one hipGraph and cg_graph_launch replay it.
//
// A plan is compiled by symbolic execution: the module tree is walked once per (input shape, training flags) with tensor
// descriptors instead of data; every launch becomes a closure over resolved pointers and geometry, appended to a flat op list.
// The tree has ONE walker, the lockstep one (gfwd / gbwd over G sibling modules): the root, or a branch without a twin, is a group of
// one and emits the plain single-module launches.  Running a pass is a loop over that list.  Random draws (dropout masks) sit at
// fixed offsets from the counter-stream position the caller passes in, in the order a module-after-module walk draws them, so
// engine and oracle masks stay bit-identical.
//
// With option "trace" the launches go to recording stubs (net_ktable.inc) instead of the GPU: tests/test_net_plan.py checks the
// planner's launch sequence, data flow and draw order on a machine without a GPU.
//
// One translation unit in three files: net_plan.h holds what a plan is made of (the descriptors Val .. Run, the launch table, the
// trace helpers), net_compiler.h the compiler (struct Compiler: the walk described above), this file the runtime (ensure_streams,
// fill_run, run_ops, sync_packs, prog_key, finding or compiling the plan of a pass) and the C ABI.
#include "net_plan.h"
#include "net_compiler.h"

// ================================================================================================ runtime + C ABI
namespace cg { extern unsigned long g_opt_epoch; }

namespace {

Net* NET(void* h) { return reinterpret_cast<Net*>(h); }

long param_numel(const Mod& m, int slot) {
    switch (m.kind) {
        case K_LINEAR: return slot == 0 ? m.ia[0] * m.ia[1] : m.ia[1];
        case K_CONV: return slot == 0 ? m.ia[0] * m.ia[1] * m.ia[2] * m.ia[3] : m.ia[1];
        case K_PRELU: return slot == 0 ? 1 : 0;
        case K_BN: return m.ia[0];
        default: return 0;
    }
}
void collect_params(Net* n, const Mod& m, vector<std::pair<float*, long>>& out) {   // gradient tensors, depth-first, weight then bias
    if (m.gw) out.push_back({m.gw, param_numel(m, 0)});
    if (m.gb) out.push_back({m.gb, param_numel(m, 1)});
    for (int c : m.kids) collect_params(n, *n->mods[c], out);
}

// Buffers the library allocated while compiling were zeroed by hipMemset on the NULL stream, which the (non-blocking) streams the
// pass runs on do not wait for: finish the memsets before the first launch can touch them.
int settle_allocs(Net* n) {
    if (n->fresh_allocs && !n->trace) CG_HIP(hipDeviceSynchronize());
    n->fresh_allocs = false;
    return 0;
}

// Side streams come out of the process-wide pool of streams classified by hardware queue (cg::queue_stream, common.h): stream index t of
// a plan runs on queue class kQueueOf[t] relative to the caller's stream - [1..3] the branch groups' streams, [4 + s] the weight-gradient
// stream beside stream s.  Measured on the batch-128 step (profiles/r05_queue_classes.txt; one box, ms per step): what must overlap has to
// sit on DIFFERENT queues - a weight-gradient stream or the host's side stream on the step's own queue costs 0.2-0.4 ms - and beyond that
// the choice is flat within 0.03 ms; D's best was its chain's weight gradients on the branch stream's queue and the branch's on a third
// (5.91 against 5.95-6.2 for the other fifteen).  (The CG_QMAP override of round 5 went with round 6's pruning: the
// assignments were swept there and the choice is flat beyond "what must overlap sits on different queues".)
static const int kQueueOf[8] = {0, 1, 2, 3, 1, 3, 2, 1};
int ensure_streams(Net* n, int nstreams, void* ref) {
    if (n->trace) return 0;
    if ((int)n->side.size() < nstreams - 1) {
        static int slots[4] = {0, 0, 0, 0};
        static std::mutex mu;                 // nets of several host threads share the pool's slot counters
        std::lock_guard<std::mutex> lk(mu);
        if (n->qmap[0] < 0) {
            for (int t = 0; t < 8; ++t) n->qmap[t] = kQueueOf[t];
        }
        while ((int)n->side.size() < nstreams - 1) {
            const int t = (int)n->side.size() + 1;
            const int c = n->qmap[t & 7];
            hipStream_t s = cg::queue_stream((hipStream_t)ref, c, slots[c]++);
            if (!s) return 1;
            hipEvent_t e;
            CG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            n->side.push_back(s); n->side_ev.push_back(e);
        }
    }
    for (int t = 0; t < 4 && nstreams > 4; ++t)
        if (!n->wg_fork_ev[t]) {
            CG_HIP(hipEventCreateWithFlags(&n->wg_fork_ev[t], hipEventDisableTiming));
            CG_HIP(hipEventCreateWithFlags(&n->wg_join_ev[t], hipEventDisableTiming));
        }
    if (!n->fork_ev) CG_HIP(hipEventCreateWithFlags(&n->fork_ev, hipEventDisableTiming));
    if (!n->pack_ev) {
        CG_HIP(hipEventCreateWithFlags(&n->pack_fork_ev, hipEventDisableTiming));
        CG_HIP(hipEventCreateWithFlags(&n->pack_ev, hipEventDisableTiming));
    }
    return 0;
}

void fill_run(Net* n, Prog* pr, Run& c, void* stream) {
    c.net = n; c.pr = pr;
    c.st[0] = (hipStream_t)stream;
    for (int t = 1; t < 8; ++t) {
        if (n->trace) c.st[t] = (hipStream_t)(uintptr_t)(0x1000 + t);
        else c.st[t] = t - 1 < (int)n->side.size() ? n->side[t - 1] : (hipStream_t)stream;
    }
    if (n->trace) { n->trace_streams.assign(8, nullptr); for (int t = 0; t < 8; ++t) n->trace_streams[t] = (void*)c.st[t]; if (!stream) n->trace_streams[0] = nullptr; }
}

// join_before: index of the first op that needs the weights sync_packs re-packed on the side stream (-1: nothing pending)
int run_ops(Net* n, vector<Op>& ops, Run& c, int join_before = -1) {
    g_cur_net = n;
    int at = 0;
    for (Op& op : ops) {
        if (at++ == join_before) {
            if (n->trace) trace_note(n, "event|wait|packs|all");
            else
                for (int t = 0; t < c.pr->nstreams; ++t)
                    if (t != 1 && hipStreamWaitEvent(c.st[t], n->pack_ev, 0) != hipSuccess) { g_cur_net = nullptr; return cg::fail("cg_net: hipStreamWaitEvent failed"); }
        }
        c.cur = op.sidx;
        const int rc = op.fn(c);
        if (rc) { g_cur_net = nullptr; cg::wgrad_discard_all(); return rc; }   // a failed pass leaves no queued reductions behind
    }
    g_cur_net = nullptr;
    return 0;
}

// Refresh the kernel-side weight copies after a parameter update: every plain layer of the net in ONE launch
// (cg_pack_conv_weight_batch), layers behind a folded upsampling with their own (phase-summed / Winograd) packing.  Only the first
// of those is needed at once: the others are packed on side stream 1 beside the head of the pass (option pack_overlap), and
// *join_before is the forward op in front of which the pass has to wait for them.
int sync_packs(Net* n, Prog* pr, Run& c, int* join_before) {
    *join_before = -1;
    if (n->params_dirty) {
        for (auto& mp : n->mods) { mp->dirty_plain = true; mp->dirty_ups = true; }
        n->params_dirty = false;
    }
    void* stream = c.S(0);
    vector<const float*> w; vector<float*> wf, wb; vector<int> co, ci, kh, kw, mp_;
    vector<Mod*> ups;
    g_cur_net = n;
    for (auto& up : n->mods) {
        Mod& m = *up;
        if (!m.is_gemm()) continue;
        if (m.wf && m.dirty_plain) {
            if (!m.w) return cg::fail("cg_net: layer %d has no weight bound (cg_net_bind)", m.id);
            w.push_back(m.w); wf.push_back(m.wf); wb.push_back(m.wb);
            if (m.pk_map == 1) { co.push_back((int)m.ia[1]); ci.push_back((int)m.map_c); kh.push_back((int)m.map_h); kw.push_back((int)m.map_w); mp_.push_back(1); }
            else if (m.kind == K_LINEAR) { co.push_back((int)m.ia[1]); ci.push_back((int)m.ia[0]); kh.push_back(1); kw.push_back(1); mp_.push_back(0); }
            else { co.push_back((int)m.ia[1]); ci.push_back((int)m.ia[0]); kh.push_back((int)m.kH()); kw.push_back((int)m.kW()); mp_.push_back(0); }
            m.dirty_plain = false;
        }
        if (m.wf_ph && m.dirty_ups) ups.push_back(&m);
    }
    if (!w.empty() && n->K->pack_conv_weight_batch(stream, (int)w.size(), w.data(), wf.data(), wb.data(), co.data(), ci.data(), kh.data(), kw.data(), mp_.data())) return 1;
    auto first_op = [&](const Mod* m) { auto it = pr->ups_first_op.find(m->id); return it == pr->ups_first_op.end() ? -1 : it->second; };
    std::stable_sort(ups.begin(), ups.end(), [&](const Mod* a, const Mod* b) { return first_op(a) < first_op(b); });   // unknown to this plan first
    const bool can_side = n->pack_overlap && c.st[1] != c.st[0];
    bool forked = false;
    for (size_t i = 0; i < ups.size(); ++i) {
        Mod& m = *ups[i];
        const int fo = first_op(&m);
        const bool on_side = can_side && i >= 1 && fo > 0 && fo < (int)pr->fwd.size();
        if (on_side && !forked) {
            forked = true;
            if (n->trace) trace_note(n, "event|record|packs_fork|s0\nevent|wait|packs_fork|s1");
            else if (hipEventRecord(n->pack_fork_ev, c.st[0]) != hipSuccess || hipStreamWaitEvent(c.st[1], n->pack_fork_ev, 0) != hipSuccess)
                return cg::fail("cg_net: cannot fork the packing stream");
        }
        void* st = on_side ? c.S(1) : stream;
        if (n->K->pack_conv_weight_ups2(st, m.w, m.wf_ph, m.wb_ph, (int)m.ia[1], (int)m.ia[0], (int)m.kH(), (int)((m.kH() - 1) / 2))) return 1;
        if (m.wino && n->K->conv2d_ups2_wino_pack(st, m.wf_ph, m.wb_ph, m.u_fwd, m.u_bwd, (int)m.ia[1], (int)m.ia[0])) return 1;
        if (m.u22 && n->K->conv2d_ups2_wino22_pack(st, m.wf_ph, m.wb_ph, m.u22, m.u22b, (int)m.ia[1], (int)m.ia[0])) return 1;
        if (on_side && (*join_before < 0 || fo < *join_before)) *join_before = fo;
        m.dirty_ups = false;
    }
    if (forked) {
        if (n->trace) trace_note(n, "event|record|packs|s1");
        else if (hipEventRecord(n->pack_ev, c.st[1]) != hipSuccess) return cg::fail("cg_net: hipEventRecord failed");
        n->pack_inflight = true;
    } else if ((!w.empty() || !ups.empty()) && !n->trace) {
        // everything was re-packed on the caller's stream (pack_overlap off, fewer than two layers behind an upsampling, no side stream):
        // a LATER pass of this net on ANOTHER stream - the side-by-side generator forward - still has to wait for it
        if (hipEventRecord(n->pack_ev, c.st[0]) != hipSuccess) return cg::fail("cg_net: hipEventRecord failed");
        n->pack_inflight = true;
    }
    g_cur_net = nullptr;
    return 0;
}

std::string prog_key(Net* n, int nd, const long* dims, int fmt) {
    std::string k = std::to_string(fmt) + ":";
    for (int i = 0; i < nd; ++i) k += std::to_string(dims[i]) + "x";
    k += "|t";
    for (auto& m : n->mods) if (m->kind == K_BN || m->kind == K_SDROP || m->kind == K_DROP) k += m->train ? '1' : '0';
    k += "|w" + std::to_string(n->world) + (n->sync_bn ? "s" : "-") + (n->bucket_overlap ? "b" : "-");
    k += "|o" + std::to_string(n->overlap_groups) + std::to_string(n->defer_wgrad) + std::to_string(n->winograd) + std::to_string(n->fusion) +
         std::to_string(n->stacking) + std::to_string(n->grouped) + std::to_string(n->share_pool) + std::to_string(n->sampler_shared) +
         std::to_string(n->view_fuse) + std::to_string(n->cat_fuse) + std::to_string(n->fuse_locnet) + std::to_string(n->head_fuse) +
         std::to_string(n->wgrad_stream) + std::to_string(n->wino22) + std::to_string(n->wino_dsplit) + "m" +
         std::to_string(n->wino_min_tiles);
    return k;
}

// The plan of a forward pass on this input shape under the net's present flags and options: found, or compiled now.
int forward_plan(Net* n, void* stream, int nd, const long* dims, int fmt, Prog** out) {
    const std::string key = prog_key(n, nd, dims, fmt);
    auto it = n->progs.find(key);
    if (it != n->progs.end() && it->second->opt_epoch != cg::g_opt_epoch) {   // cg_set_option moved the dispatch
        if (n->last == it->second.get()) n->last = nullptr;   // a failed recompile must not leave backward a dangling plan
        n->progs.erase(it); it = n->progs.end();
    }
    if (it == n->progs.end()) {
        std::unique_ptr<Prog> pr(new Prog());
        pr->net = n; pr->opt_epoch = cg::g_opt_epoch;
        Val in; in.none = false; in.ext = EXT_X; in.nd = nd; for (int i = 0; i < nd; ++i) in.d[i] = dims[i]; in.fmt = fmt;
        pr->in = in;
        Compiler C(n, pr.get());
        C.ops = &pr->fwd;
        Compiler::GCtx ctx{{C.rng}};   // the root module: a group of one at the start of the pass's draws
        pr->out = C.gfwd({n->mods[0].get()}, {in}, ctx)[0];
        if (C.failed) return cg::fail("%s", n->err);
        CG_REQUIRE(!pr->out.is_tab, "cg_net_forward: the root module returns a table");
        pr->out = C.materialise(pr->out);
        pr->draws = ctx.cur[0];
        if (ensure_streams(n, std::max(pr->nstreams, n->pack_overlap && pr->ups_first_op.size() >= 2 ? 2 : 1), stream)) return 1;
        if (settle_allocs(n)) return 1;
        it = n->progs.emplace(key, std::move(pr)).first;
    }
    *out = it->second.get();
    return 0;
}

// Gradient buckets of the root nn.Sequential: contiguous ranges of the flat gradient, a conv / linear layer with the parameters of the
// modules up to the next one (none when the bound gradient tensors are not one contiguous vector in module order).
void make_buckets(Net* n, Prog* pr) {
    const Mod& root = *n->mods[0];
    bool contiguous = true; float* expect = nullptr;
    for (size_t i = 0; i < root.kids.size(); ++i) {
        vector<std::pair<float*, long>> ps;
        collect_params(n, *n->mods[root.kids[i]], ps);
        long cnt = 0; for (auto& p : ps) cnt += p.second;
        if (n->mods[root.kids[i]]->is_gemm() || pr->buckets.empty()) {
            if (ps.empty() && pr->buckets.empty()) continue;
            pr->buckets.push_back({ps.empty() ? expect : ps[0].first, 0}); pr->bucket_first.push_back((int)i);
        }
        for (auto& p : ps) { if (expect && p.first != expect) contiguous = false; expect = p.first + p.second; }
        pr->buckets.back().second += cnt;
    }
    if (!contiguous) { pr->buckets.clear(); pr->bucket_first.clear(); }
    // buckets below 256 KB ride with the one the backward completes next (a collective costs a launch and a latency whatever it
    // carries): G's last convolution (3 459 values) with the 256 -> 128 layer, D's head with Linear(20480, 256), D's first layers
    // in one exchange at the end
    constexpr long kMinBucket = 65536;
    vector<std::pair<float*, long>> mb; vector<int> mf;
    long accn = 0;
    for (int j = (int)pr->buckets.size() - 1; j >= 0; --j) {
        accn += pr->buckets[j].second;
        if (accn >= kMinBucket || j == 0) {
            mb.insert(mb.begin(), {pr->buckets[j].first, accn}); mf.insert(mf.begin(), pr->bucket_first[j]);
            accn = 0;
        }
    }
    pr->buckets.swap(mb); pr->bucket_first.swap(mf);
}

// Compile the backward of the plan the last forward ran: acc 1 Module:backward (gradInput + accGradParameters), 0 updateGradInput only.
int compile_backward(Net* n, Prog* pr, void* stream, int acc, int gy_fmt) {
    Compiler C(n, pr);
    C.ops = &pr->bwd[acc];
    C.acc_pass = acc != 0;
    pr->bwd[acc].clear();
    Mod& root = *n->mods[0];
    if (acc && n->bucket_overlap && n->world > 1 && root.kind == K_SEQ && root.kids.size() > 1 && pr->buckets.empty()) make_buckets(n, pr);
    C.bucket_done_upto = (int)root.kids.size();
    Val go = pr->out; go.ext = EXT_GY; go.off = 0; go.p = nullptr; go.fmt = gy_fmt; go.blk = 0; go.gi = go.gc = 0;
    Val gi = C.gbwd({&root}, {pr->in}, {go}, acc != 0, true)[0];
    if (C.failed) return cg::fail("%s", n->err);
    if (acc) { C.buckets_start(); C.flush_wgrad(); C.wg_join_all(); }
    CG_REQUIRE(!gi.is_tab, "cg_net_backward: the root module's gradInput is a table");
    pr->gin[acc] = gi;
    pr->have_bwd[acc] = true;
    if (ensure_streams(n, pr->nstreams, stream)) return 1;
    return settle_allocs(n);
}

// A tensor of a plan to the caller: its address, its logical shape, its layout code (fmt, or fmt + 2 * ups where a lazily upsampled one may leave)
void put_val(const Val& v, float* p, int fmt, float** ptr, int* nd, long* dims, int* fmtp) {
    if (ptr) *ptr = p;
    if (nd) *nd = v.nd;
    if (dims) for (int i = 0; i < 4; ++i) dims[i] = v.d[i];
    if (fmtp) *fmtp = fmt;
}

}  // namespace

extern "C" {

int cg_net_create(void** net) {
    CG_REQUIRE(net, "cg_net_create: null pointer");
    Net* n = new Net();
    *net = n;
    // CG_NET_OPTIONS="name=value,name=value": plan options of EVERY net of the process, through cg_net_set_option below (same-box A/B runs
    // of bench.py; round 5 folded the eighteen per-option variables - CG_WINOGRAD22, CG_WGRAD_STREAM, CG_FUSION ... - into this one)
    if (const char* e = getenv("CG_NET_OPTIONS")) {
        std::string all(e);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string kv = all.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || eq == 0) { delete n; *net = nullptr; return cg::fail("CG_NET_OPTIONS: expected name=value, got '%s'", kv.c_str()); }
            if (cg_net_set_option(n, kv.substr(0, eq).c_str(), atol(kv.c_str() + eq + 1))) { delete n; *net = nullptr; return 1; }
            pos = end + 1;
        }
    }
    return 0;
}

int cg_net_destroy(void* net) {
    Net* n = NET(net);
    if (!n) return 0;
    for (void* p : n->owned) { if (n->trace) free(p); else (void)hipFree(p); }
    // n->side: pool streams (cg::queue_stream), not ours to destroy
    for (auto e : n->side_ev) (void)hipEventDestroy(e);
    if (n->fork_ev) (void)hipEventDestroy(n->fork_ev);
    if (n->pack_ev) { (void)hipEventDestroy(n->pack_fork_ev); (void)hipEventDestroy(n->pack_ev); }
    if (n->pair_fork_ev) { (void)hipEventDestroy(n->pair_fork_ev); (void)hipEventDestroy(n->pair_a_ev); (void)hipEventDestroy(n->pair_join_ev); }
    for (int t = 0; t < 4; ++t) if (n->wg_fork_ev[t]) { (void)hipEventDestroy(n->wg_fork_ev[t]); (void)hipEventDestroy(n->wg_join_ev[t]); }
    delete n;
    return 0;
}

int cg_net_set_option(void* net, const char* name, long value) {
    Net* n = NET(net);
    CG_REQUIRE(n && name, "cg_net_set_option: null pointer");
    struct { const char* nm; int* p; } tab[] = {
        {"overlap_groups", &n->overlap_groups}, {"defer_wgrad", &n->defer_wgrad}, {"winograd", &n->winograd}, {"share_pool", &n->share_pool},
        {"sampler_shared", &n->sampler_shared}, {"view_fuse", &n->view_fuse}, {"cat_fuse", &n->cat_fuse}, {"stacking", &n->stacking},
        {"grouped", &n->grouped}, {"fusion", &n->fusion}, {"fuse_locnet", &n->fuse_locnet}, {"pack_overlap", &n->pack_overlap},
        {"head_fuse", &n->head_fuse}, {"wgrad_stream", &n->wgrad_stream}, {"wino_dsplit", &n->wino_dsplit}};
    if (!strcmp(name, "trace")) {
        CG_REQUIRE(n->progs.empty(), "cg_net_set_option: trace must be chosen before the first pass");
        n->trace = value != 0; n->K = n->trace ? &kTraceTable : &kRealTable;
        return 0;
    }
    if (!strcmp(name, "defer_running")) { n->defer_running = value != 0; return 0; }   // run-time switch, plans unchanged
    if (!strcmp(name, "winograd_min_tiles")) { n->wino_min_tiles = value; return 0; }
    if (!strcmp(name, "winograd22")) { n->wino22 = (int)value & 3; return 0; }     // bit mask: 1 forward, 2 data gradient
    if (!strcmp(name, "fuse_locnet")) { n->fuse_locnet = (int)value; return 0; }   // 0 off, 1 every localisation branch, 2 ungrouped ones only
    for (auto& t : tab) if (!strcmp(name, t.nm)) { *t.p = value != 0; return 0; }
    return cg::fail("cg_net_set_option: unknown option %s", name);
}

int cg_net_set_allocator(void* net, cg_alloc_fn alloc, void* user) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_set_allocator: null net");
    n->alloc_fn = alloc; n->alloc_user = user;
    return 0;
}

int cg_net_set_hook(void* net, cg_hook_fn hook, void* user) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_set_hook: null net");
    n->hook = hook; n->hook_user = user;
    return 0;
}

int cg_net_set_dp(void* net, int world, int sync_bn, void* comm_bn, void* comm_grad, int bucket_overlap) {
    Net* n = NET(net);
    CG_REQUIRE(n && world >= 1, "cg_net_set_dp: bad arguments");
    n->world = world; n->sync_bn = sync_bn != 0; n->comm_bn = comm_bn; n->comm_grad = comm_grad; n->bucket_overlap = (bucket_overlap & 1) != 0;
    n->hook_too = (bucket_overlap & 2) != 0;
    return 0;
}

int cg_net_add(void* net, int parent, int kind, const long* iargs, int niargs, const float* fargs, int nfargs, int* id) {
    Net* n = NET(net);
    CG_REQUIRE(n && id, "cg_net_add: null pointer");
    CG_REQUIRE(kind >= 0 && kind < K_COUNT, "cg_net_add: unknown module kind %d", kind);
    CG_REQUIRE(niargs <= 8 && nfargs <= 4, "cg_net_add: too many arguments");
    CG_REQUIRE(parent < (int)n->mods.size(), "cg_net_add: unknown parent %d", parent);
    CG_REQUIRE((parent < 0) == n->mods.empty(), "cg_net_add: exactly the first module is the root (parent -1)");
    if (parent >= 0) CG_REQUIRE(n->mods[parent]->is_container(), "cg_net_add: parent %d is not a container", parent);
    std::unique_ptr<Mod> m(new Mod());
    m->id = (int)n->mods.size(); m->kind = kind; m->parent = parent;
    for (int i = 0; i < niargs; ++i) m->ia[i] = iargs[i];
    for (int i = 0; i < nfargs; ++i) m->fa[i] = fargs[i];
    if (kind == K_VIEW) m->ia[7] = niargs;
    if (kind == K_CONV) CG_REQUIRE(m->ia[6] <= 1 && m->ia[7] <= 1, "cg_net_add: only stride 1 convolutions are on the path");
    if (kind == K_CONCAT) CG_REQUIRE(m->ia[0] == 2, "cg_net_add: nn.Concat joins on dimension 2 (channels)");
    if (parent >= 0) n->mods[parent]->kids.push_back(m->id);
    *id = m->id;
    n->mods.push_back(std::move(m));
    n->progs.clear(); n->last = nullptr;
    return 0;
}

int cg_net_bind(void* net, int id, int slot, float* param, float* grad) {
    Net* n = NET(net);
    CG_REQUIRE(n && id >= 0 && id < (int)n->mods.size(), "cg_net_bind: unknown module %d", id);
    Mod& m = *n->mods[id];
    if (slot == 0) { m.w = param; m.gw = grad; }
    else if (slot == 1) { m.b = param; m.gb = grad; }
    else if (slot == 2) { m.rmean = param; m.rvar = grad; }
    else return cg::fail("cg_net_bind: slot %d (0 weight, 1 bias, 2 running mean / var)", slot);
    n->params_dirty = true;
    for (auto& kv : n->progs) { kv.second->buckets.clear(); kv.second->bucket_first.clear(); kv.second->have_bwd[1] = false; kv.second->bwd[1].clear(); }
    return 0;
}

int cg_net_set_training(void* net, int id, int train) {
    Net* n = NET(net);
    CG_REQUIRE(n && id < (int)n->mods.size(), "cg_net_set_training: unknown module %d", id);
    if (id < 0) for (auto& m : n->mods) m->train = train != 0;
    else n->mods[id]->train = train != 0;
    return 0;
}

int cg_net_params_changed(void* net) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_params_changed: null net");
    n->params_dirty = true;
    return 0;
}

int cg_net_trace_region(void* net, const void* base, size_t bytes) {
    Net* n = NET(net);
    CG_REQUIRE(n && base, "cg_net_trace_region: null pointer");
    n->regions.push_back(Region{(const char*)base, bytes});
    return 0;
}

int cg_net_trace_take(void* net, char* out, size_t cap, size_t* len) {
    Net* n = NET(net);
    CG_REQUIRE(n && len, "cg_net_trace_take: null pointer");
    *len = n->trace_log.size();
    if (out && cap >= n->trace_log.size()) { memcpy(out, n->trace_log.data(), n->trace_log.size()); n->trace_log.clear(); }
    return 0;
}

int cg_net_forward(void* net, void* stream, const float* x, int nd, const long* dims, int fmt, uint64_t rng_seed, uint64_t rng_offset,
                   const uint64_t* rng_base, uint64_t* draws, float** y, int* ynd, long* ydims, int* yfmt) {
    Net* n = NET(net);
    CG_REQUIRE(n && x && dims && nd >= 1 && nd <= 4, "cg_net_forward: bad arguments");
    CG_REQUIRE(!n->mods.empty(), "cg_net_forward: empty net");
    Prog* pr = nullptr;
    if (forward_plan(n, stream, nd, dims, fmt, &pr)) return 1;
    Run c;
    fill_run(n, pr, c, stream);
    int join_before = -1;
    if (sync_packs(n, pr, c, &join_before)) return 1;
    // another pass of this net (on another stream) may have the re-packing in flight: wait for it before the first launch
    if (join_before < 0 && n->pack_inflight && !n->trace && hipStreamWaitEvent(c.st[0], n->pack_ev, 0) != hipSuccess)
        return cg::fail("cg_net_forward: hipStreamWaitEvent failed");
    c.x = x; c.seed = rng_seed; c.roff = rng_offset; c.rbase = rng_base;
    if (run_ops(n, pr->fwd, c, join_before)) return 1;
    n->last = pr;
    pr->running_pending = n->defer_running != 0 && !pr->bn_runs.empty();
    if (draws) *draws = (uint64_t)pr->draws;
    put_val(pr->out, c.P(pr->out), pr->out.fmt, y, ynd, ydims, yfmt);
    return 0;
}

int cg_net_backward(void* net, void* stream, const float* x, const float* gy, int gy_fmt, int acc, float scale, float** gx, int* gnd, long* gdims,
                    int* gfmt) {
    Net* n = NET(net);
    CG_REQUIRE(n && x && gy, "cg_net_backward: null pointer");
    Prog* pr = n->last;
    CG_REQUIRE(pr, "cg_net_backward: no forward pass to continue");
    acc = acc ? 1 : 0;
    if (!pr->have_bwd[acc] && compile_backward(n, pr, stream, acc, gy_fmt)) return 1;
    Run c;
    fill_run(n, pr, c, stream);
    c.x = x; c.gy = gy; c.scale = scale;
    n->pack_inflight = false;      // every forward pass since the last re-packing has waited for it
    if (run_ops(n, pr->bwd[acc], c)) return 1;
    const Val& gi = pr->gin[acc];
    put_val(gi, c.P(gi), gi.fmt + 2 * gi.ups, gx, gnd, gdims, gfmt);
    return 0;
}

int cg_net_apply_running(void* net, void* stream) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_apply_running: null net");
    Prog* pr = n->last;
    if (!pr || !pr->running_pending) return 0;
    pr->running_pending = false;
    g_cur_net = n;
    for (auto& b : pr->bn_runs) {
        if (!b.bn->rmean || !b.bn->rvar) continue;
        if (n->K->bn_running_update(stream, (const double*)b.sums.p, b.cnt, (int)b.C, b.mom, b.bn->rmean, b.bn->rvar)) { g_cur_net = nullptr; return 1; }
    }
    g_cur_net = nullptr;
    return 0;
}

// Two forward passes of ONE net side by side (SURVEY.md 8b "optional coarse entry"): adversarial.lua:232-233 runs MODEL_G on
// the D-step's N/2 noise rows and :185 on the G-step's N rows, and MODEL_G moves only at :262 - both passes read the same parameters.  Pass
// 1 runs on the caller's stream exactly as cg_net_forward would; pass 2 (its input must already be enqueued on `stream`) runs on a
// library stream of ANOTHER hardware queue, leaves the batch-norm running statistics alone and applies its update behind pass 1's, so
// that results, running statistics and the plan cg_net_backward continues (pass 2's) are those of forward(x) followed by forward(x2).
// The caller's stream does not wait for pass 2 until cg_net_pair_join, which also hands out pass 2's output.  draws = both passes'.
int cg_net_forward_pair(void* net, void* stream, const float* x, int nd, const long* dims, int fmt, const float* x2, int nd2, const long* dims2,
                        int fmt2, uint64_t rng_seed, uint64_t rng_offset, const uint64_t* rng_base, uint64_t* draws, float** y, int* ynd,
                        long* ydims, int* yfmt) {
    Net* n = NET(net);
    CG_REQUIRE(n && x && x2 && dims && dims2, "cg_net_forward_pair: null pointer");
    CG_REQUIRE(!n->pair_pending, "cg_net_forward_pair: the previous pair was never joined (cg_net_pair_join)");
    if (n->trace) {      // a trace records the launches of both passes one after the other
        uint64_t d1 = 0, d2 = 0;
        if (cg_net_forward(net, stream, x, nd, dims, fmt, rng_seed, rng_offset, rng_base, &d1, y, ynd, ydims, yfmt)) return 1;
        trace_note(n, "pair|second pass on the pair stream");
        if (cg_net_forward(net, stream, x2, nd2, dims2, fmt2, rng_seed, rng_offset + d1, rng_base, &d2, &n->pair_y, nullptr, nullptr, nullptr)) return 1;
        if (draws) *draws = d1 + d2;
        n->pair_out = n->last->out; n->pair_pending = true;
        return 0;
    }
    if (!n->pair_fork_ev) {
        n->pair_stream = cg::queue_stream(cg::S(stream), 2, 7);     // any class but the caller's own measures the same (profiles/r05_queue_classes.txt)
        if (!n->pair_stream) return 1;
        CG_HIP(hipEventCreateWithFlags(&n->pair_fork_ev, hipEventDisableTiming));
        CG_HIP(hipEventCreateWithFlags(&n->pair_a_ev, hipEventDisableTiming));
        CG_HIP(hipEventCreateWithFlags(&n->pair_join_ev, hipEventDisableTiming));
    }
    hipStream_t st = cg::S(stream), side = n->pair_stream;
    CG_HIP(hipEventRecord(n->pair_fork_ev, st));
    CG_HIP(hipStreamWaitEvent(side, n->pair_fork_ev, 0));
    uint64_t d1 = 0, d2 = 0;
    if (cg_net_forward(net, stream, x, nd, dims, fmt, rng_seed, rng_offset, rng_base, &d1, y, ynd, ydims, yfmt)) return 1;
    CG_HIP(hipEventRecord(n->pair_a_ev, st));      // pass 1, its running-statistics update included, is complete on the caller's stream
    const int defer = n->defer_running;
    n->defer_running = 1;
    const int rc = cg_net_forward(net, (void*)side, x2, nd2, dims2, fmt2, rng_seed, rng_offset + d1, rng_base, &d2, &n->pair_y, nullptr, nullptr, nullptr);
    n->defer_running = defer;
    if (rc) return 1;
    CG_HIP(hipStreamWaitEvent(side, n->pair_a_ev, 0));
    if (cg_net_apply_running(net, (void*)side)) return 1;      // off the caller's chain, but behind pass 1's update: the reference's order
    CG_HIP(hipEventRecord(n->pair_join_ev, side));
    n->pair_out = n->last->out; n->pair_pending = true;
    if (draws) *draws = d1 + d2;
    return 0;
}

int cg_net_pair_join(void* net, void* stream, float** y, int* ynd, long* ydims, int* yfmt) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_pair_join: null net");
    CG_REQUIRE(n->pair_pending, "cg_net_pair_join: no pair in flight");
    if (!n->trace) CG_HIP(hipStreamWaitEvent(cg::S(stream), n->pair_join_ev, 0));
    n->pair_pending = false;
    put_val(n->pair_out, n->pair_y, n->pair_out.fmt, y, ynd, ydims, yfmt);
    return 0;
}

int cg_net_buckets(void* net, int* nbuckets) {
    Net* n = NET(net);
    CG_REQUIRE(n && nbuckets, "cg_net_buckets: null pointer");
    *nbuckets = n->last ? (int)n->last->buckets.size() : 0;
    return 0;
}

int cg_net_module_state(void* net, int id, int which, float** ptr, int* nd, long* dims, int* fmt) {
    Net* n = NET(net);
    CG_REQUIRE(n && ptr && id >= 0 && id < (int)n->mods.size(), "cg_net_module_state: bad arguments");
    *ptr = nullptr;
    if (!n->last) return 0;
    auto it = n->last->ms.find(id);
    if (it == n->last->ms.end()) return 0;
    const Val& v = which == 0 ? it->second.out : which == 1 ? it->second.gin : it->second.noise;
    if (v.none || v.is_tab || v.ext) return 0;
    put_val(v, v.p, v.fmt + 2 * v.ups, ptr, nd, dims, fmt);
    return 0;
}

int cg_net_stats(void* net, long* nprograms, long* nlaunch_fwd, long* nlaunch_bwd, size_t* bytes) {
    Net* n = NET(net);
    CG_REQUIRE(n, "cg_net_stats: null net");
    if (nprograms) *nprograms = (long)n->progs.size();
    if (nlaunch_fwd) *nlaunch_fwd = n->last ? (long)n->last->fwd.size() : 0;
    if (nlaunch_bwd) *nlaunch_bwd = n->last ? (long)std::max(n->last->bwd[0].size(), n->last->bwd[1].size()) : 0;
    if (bytes) { size_t b = 0; for (auto& r : n->regions) b += r.bytes; *bytes = b; }
    return 0;
}

// ---- whole-iteration capture: the host runs its training iteration once between begin and end (every launch it makes on `stream`,
// and on streams forked from it by events, is recorded instead of executed), then replays the graph per step.
int cg_graph_begin(void* stream) {
    CG_HIP(hipStreamBeginCapture(cg::S(stream), hipStreamCaptureModeRelaxed));
    return 0;
}
int cg_graph_end(void* stream, void** graph_exec) {
    CG_REQUIRE(graph_exec, "cg_graph_end: null pointer");
    hipGraph_t g = nullptr;
    CG_HIP(hipStreamEndCapture(cg::S(stream), &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return cg::fail("cg_graph_end: hipGraphInstantiate -> %s", hipGetErrorString(e));
    *graph_exec = (void*)ex;
    return 0;
}
int cg_graph_launch(void* graph_exec, void* stream) {
    CG_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, cg::S(stream)));
    return 0;
}
int cg_graph_destroy(void* graph_exec) {
    if (graph_exec) CG_HIP(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return 0;
}

}  // extern "C"
