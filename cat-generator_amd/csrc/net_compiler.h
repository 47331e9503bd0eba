// net_compiler.h - the plan compiler of the planned executor: struct Compiler and nothing else (included by net.hip behind net_plan.h).
//
// One Compiler walks the module tree once per (plan, pass) and appends the pass's launches, as closures over resolved pointers and
// geometry, to an op list of the Prog.  In the order of the file: memory and layout helpers, conv / linear preparation and the GEMM
// emitters every form of a layer goes through, forward of one module, lockstep forward of sibling modules, the fused segments of
// nn.Sequential, the fused localisation branch, nn.Concat with its streams, backward, the data-parallel exchanges.
#pragma once

namespace {

struct Compiler {
    struct GCtx { vector<long> cur; };   // per-branch positions in the counter stream during a lockstep walk (a lone module: one branch)

    struct Prep { Val x; int wsel; Val out; Geo g; bool ok = true; };
    enum { W_PLAIN_F = 0, W_PH_F, W_PLAIN_B, W_PH_B, W_CANON };
    static float* wsel(const Mod* m, int sel) {
        switch (sel) {
            case W_PLAIN_F: return m->wf;
            case W_PH_F: return m->wf_ph;
            case W_PLAIN_B: return m->wb ? m->wb : m->w;
            case W_PH_B: return m->wb_ph;
            default: return m->w;
        }
    }

    Net* net;
    Prog* pr;
    vector<Op>* ops = nullptr;
    int cs = 0;              // stream index launches are emitted on
    long rng = 0;            // counter-stream position (relative to the pass's start) of the branch whose module is being emitted (per_branch)
    int dry = 0;             // > 0: shape / draw bookkeeping only (no allocation, no ops, no module state kept)
    bool failed = false;
    int pend[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // deferred weight-gradient reductions queued per stream index
    bool wg_used[4] = {false, false, false, false};   // the weight-gradient stream beside stream s has work to join
    bool wg_unjoined[4] = {false, false, false, false};   // ... that no gradient bucket has waited for yet
    bool acc_pass = false;        // compiling Module:backward (weight gradients deferred) rather than updateGradInput

    Compiler(Net* n, Prog* p) : net(n), pr(p) {}
    const KTable* K() const { return net->K; }
    Mod& M(int id) { return *net->mods[id]; }
    MS& S(const Mod& m) { return pr->ms[m.id]; }
    int err(const char* fmt, ...) {
        va_list ap; va_start(ap, fmt); vsnprintf(net->err, sizeof net->err, fmt, ap); va_end(ap);
        failed = true;
        return 1;
    }

    // ---------------------------------------------------------------------------------------- memory
    void* alloc(size_t bytes) {
        if (dry) return nullptr;
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes == 0) bytes = 256;
        void* p = nullptr;
        if (net->trace) {
            p = calloc(1, bytes);   // never dereferenced by the recording stubs; a real address keeps regions disjoint
        } else if (net->alloc_fn) {
            p = net->alloc_fn(net->alloc_user, bytes);      // host allocator: zero-initialised device memory
        } else {
            // the memset is ordered on the null stream only: cg_net_forward / _backward synchronise once after compiling (fresh_allocs)
            if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) p = nullptr;
            else net->fresh_allocs = true;
        }
        if (!p) { err("cg_net: allocation of %zu bytes failed", bytes); return nullptr; }
        if (!net->alloc_fn || net->trace) net->owned.push_back(p);
        net->regions.push_back(Region{(const char*)p, bytes});
        return p;
    }
    Val anon(std::initializer_list<long> dims, int fmt = PLAIN) {
        long n = 1; for (long x : dims) n *= x;
        Val v = mkval((float*)alloc((size_t)n * 4), dims, fmt);
        return v;
    }
    Val anon_like(const Val& x, int fmt) {
        Val v = x; v.p = (float*)alloc((size_t)x.numel() * 4); v.ext = 0; v.off = 0; v.fmt = fmt; v.ups = 0; v.blk = 0; v.gi = v.gc = 0;
        return v;
    }
    // Module._get: one persistent buffer per (module, role, element count)
    Val buf(const Mod& m, const std::string& role, std::initializer_list<long> dims, int fmt = PLAIN, size_t elem = 4) {
        long n = 1; for (long x : dims) n *= x;
        std::string key = role + "#" + std::to_string(n);
        MS& s = S(m);
        auto it = s.bufs.find(key);
        if (it == s.bufs.end()) {
            Val v = mkval((float*)alloc((size_t)n * elem), dims, fmt);
            s.bufs[key] = v;
            return v;
        }
        Val& b = it->second;
        Val want = mkval(nullptr, dims, fmt);
        if (!b.same_shape(want) || b.fmt != fmt) {
            const bool keep = want.nd && b.nd && want.d[0] == b.d[0];
            Val nb = reshape(b, dims, fmt, 0, keep);
            b = nb;
        }
        return b;
    }
    Val buf_like(const Mod& m, const std::string& role, const Val& like, int fmt) {
        switch (like.nd) {
            case 1: return buf(m, role, {like.d[0]}, fmt);
            case 2: return buf(m, role, {like.d[0], like.d[1]}, fmt);
            case 3: return buf(m, role, {like.d[0], like.d[1], like.d[2]}, fmt);
            default: return buf(m, role, {like.d[0], like.d[1], like.d[2], like.d[3]}, fmt);
        }
    }
    void ws_need(size_t bytes) {   // Workspace.get: grow-only scratch of the current stream
        if (dry) return;
        if (bytes < 4096) bytes = 4096;
        if ((int)pr->ws.size() <= cs) { pr->ws.resize(cs + 1, nullptr); pr->ws_bytes.resize(cs + 1, 0); }
        if (pr->ws_bytes[cs] < bytes) {
            size_t nb = bytes + bytes / 4;
            pr->ws[cs] = alloc(nb);
            pr->ws_bytes[cs] = nb;
        }
    }
    template <class F> void emit(F f) {
        if (dry) return;
        ops->push_back(Op{cs, std::function<int(Run&)>(f)});
    }
    void use_stream(int sidx) { if (!dry && sidx + 1 > pr->nstreams) pr->nstreams = sidx + 1; }

    // ---------------------------------------------------------------------------------------- layout helpers
    Val materialise(const Val& x) {
        if (!x.ups) return x;
        long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
        Val out = anon({N, C, H, W}, NHWC);
        const KTable* k = K();
        emit([=](Run& c) { return k->upsample2x_forward(c.CS(), c.P(x), c.P(out), (int)N, (int)(H >> 1), (int)(W >> 1), (int)C); });
        return out;
    }
    // NOTE: closures never read Compiler state at run time; the stream index an op was emitted on (Op::sidx) reaches the closure
    // through Run::cur, set by the runner before each op (Run::CS() = that stream, Run::W() its scratch).

    Val as_nhwc(const Val& x, bool keep_ups = false) {
        if (x.fmt == NHWC) return (keep_ups || !x.ups) ? x : materialise(x);
        if (x.nd != 4) { err("cg_net: expected a 4-D feature map"); return x; }
        long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
        Val out = anon({N, C, H, W}, NHWC);
        const KTable* k = K();
        emit([=](Run& c) { return k->nchw_to_nhwc(c.CS(), c.P(x), c.P(out), (int)N, (int)C, (int)H, (int)W); });
        return out;
    }
    Val as_plain(const Val& x0) {
        if (x0.fmt == PLAIN) return x0;
        Val x = materialise(x0);
        long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
        Val out = anon({N, C, H, W}, PLAIN);
        const KTable* k = K();
        emit([=](Run& c) { return k->nhwc_to_nchw(c.CS(), c.P(x), c.P(out), (int)N, (int)C, (int)H, (int)W); });
        return out;
    }
    void emit_scaled_copy(const Val& dst, const Val& src, float f) {   // dst = f * src (dropout in evaluate() mode), a copy and a scaling in place
        const KTable* k = K();
        const long n = src.phys();
        emit([=](Run& c) { return k->memcpy_d2d(c.CS(), c.P(dst), c.P(src), (size_t)n * 4); });
        emit([=](Run& c) { return k->scale(c.CS(), c.P(dst), f, n); });
    }
    Val match_fmt(const Val& g, const Val& like) {
        if (g.fmt == like.fmt) return g;
        return like.fmt == NHWC ? as_nhwc(g) : as_plain(g);
    }

    // ---------------------------------------------------------------------------------------- stacking of identical branches
    vector<Val> split(const Val& Y, int G) {   // a stacked tensor ([G*N, ...], branch-major) as its G per-branch slices
        vector<Val> out;
        const long n = Y.phys() / G, N = Y.d[0] / G;
        for (int i = 0; i < G; ++i) {
            Val v = Y.at((size_t)i * n * 4);
            v.d[0] = N; v.blk = Y.key(); v.gi = i; v.gc = G;
            out.push_back(v);
        }
        return out;
    }
    bool stacked(const vector<Val>& xs, Val* out) {   // the block behind G per-branch tensors if they are exactly its slices in order
        if (xs.empty() || xs[0].is_tab || xs[0].none || !xs[0].blk || xs[0].gc != (int)xs.size()) return false;
        const Val& x0 = xs[0];
        for (size_t i = 0; i < xs.size(); ++i) {
            const Val& x = xs[i];
            if (x.is_tab || x.none || x.blk != x0.blk || x.gi != (int)i || !x.same_shape(x0) || x.fmt != x0.fmt || x.ups) return false;
        }
        if (out) {
            Val b = x0;   // slice 0 starts where the block starts
            b.d[0] = x0.d[0] * (long)xs.size(); b.blk = 0; b.gi = b.gc = 0;
            *out = b;
        }
        return true;
    }
    void seed_slices(const vector<Mod*>& mods, const std::string& role, const Val& shape_of, int fmt) {
        const int G = (int)mods.size();
        const long n = shape_of.numel();
        std::string key = role + "#" + std::to_string(n);
        vector<Val> cur; bool all = true;
        for (Mod* m : mods) {
            auto it = S(*m).bufs.find(key);
            if (it == S(*m).bufs.end() || !it->second.same_shape(shape_of) || it->second.fmt != fmt) { all = false; break; }
            cur.push_back(it->second);
        }
        if (all && stacked(cur, nullptr)) return;
        Val bs = shape_of; bs.d[0] *= G;
        Val block = buf_like(*mods[0], role + ".block", bs, fmt);
        vector<Val> sl = split(block, G);
        for (int i = 0; i < G; ++i) S(*mods[i]).bufs[key] = sl[i];
    }
    Val restack(const Mod& owner, vector<Val> xs, const Val& like) {   // copy G per-branch tensors into one block
        for (auto& x : xs) x = match_fmt(x, like);
        Val bs = xs[0]; bs.d[0] *= (long)xs.size(); bs.ups = 0;
        Val block = buf_like(owner, "restack.block", bs, xs[0].fmt);
        const size_t nb = (size_t)xs[0].phys() * 4;
        const KTable* k = K();
        for (size_t i = 0; i < xs.size(); ++i) {
            Val dst = block.at(i * nb), src = xs[i];
            emit([=](Run& c) { return k->memcpy_d2d(c.CS(), c.P(dst), c.P(src), nb); });
        }
        return block;
    }

    // ---------------------------------------------------------------------------------------- kernel-side weight copies
    // Allocated when a plan first needs them; refreshed at the start of the next pass after cg_net_params_changed (one batched
    // launch for the plain layers, cg_pack_conv_weight_ups2 (+ Winograd) for layers behind a folded upsampling).
    void need_plain(Mod& m, bool map, long C = 0, long H = 0, long W = 0) {
        if (dry) return;
        const size_t n = cg_pack_conv_weight_floats((int)m.ia[1], (int)m.ia[0], (int)m.kH(), (int)m.kW());   // nn.Linear: kH = kW = 1
        const long taps = map ? H * W : m.kH() * m.kW();
        const int want = map ? 1 : 0;
        if (m.pk_map == want && (!map || (m.map_c == C && m.map_h == H && m.map_w == W))) return;
        if (!m.wf) m.wf = (float*)alloc(n * 4);
        if (taps > 1 && !m.wb) m.wb = (float*)alloc(n * 4);
        if (taps <= 1) m.wb = nullptr;     // 1x1 / linear: the canonical [out][in] matrix already is the backward operand
        m.pk_map = want; m.map_c = C; m.map_h = H; m.map_w = W;
        m.dirty_plain = true;
    }
    void need_ups(Mod& m, bool wino) {
        if (dry) return;
        if (ops == &pr->fwd && !pr->ups_first_op.count(m.id)) pr->ups_first_op[m.id] = (int)ops->size();
        if (!m.wf_ph) {
            const size_t n = cg_pack_conv_weight_ups2_floats((int)m.ia[1], (int)m.ia[0], (int)m.kH(), (int)((m.kH() - 1) / 2));
            m.wf_ph = (float*)alloc(n * 4); m.wb_ph = (float*)alloc(n * 4);
            m.dirty_ups = true;
        }
        if (wino && !m.wino) {
            m.wino = true;
            const size_t nu = cg_conv2d_ups2_wino_u_floats((int)m.ia[0], (int)m.ia[1]);
            m.u_fwd = (float*)alloc(nu * 4); m.u_bwd = (float*)alloc(nu * 4);
            m.dirty_ups = true;
        }
    }

    // ---------------------------------------------------------------------------------------- conv / linear preparation
    static bool can_fold_ups(const Mod& m) { return m.kH() == m.kW() && m.kH() % 2 == 1 && m.padH() == m.padW() && m.padH() == (m.kH() - 1) / 2; }
    bool use_wino22(Mod& m, const Val& x) {   // F(2x2,2x2) forward for a lazily upsampled input: 3x3, pad 1, even low-res grid, planes % 128
        if (!(net->winograd && (net->wino22 & 1) && m.kind == K_CONV && x.ups && m.kH() == 3 && m.kW() == 3 && m.padH() == 1 && m.padW() == 1)) return false;
        const long N = x.d[0], Hp = x.d[2] >> 1, Wp = x.d[3] >> 1;
        if (N * Hp * Wp / 4 < net->wino_min_tiles) return false;
        return cg_conv2d_ups2_wino22_supported((int)N, (int)Hp, (int)Wp, (int)m.ia[0], (int)m.ia[1]) != 0;
    }
    bool use_wino(Mod& m, const Val& x) {   // Winograd path for a lazily upsampled input: 5x5, pad 2, even low-res grid, planes % 128
        if (!(net->winograd && m.kind == K_CONV && x.ups && m.kH() == 5 && m.kW() == 5 && m.padH() == 2 && m.padW() == 2)) return false;
        const long N = x.d[0], Hp = x.d[2] >> 1, Wp = x.d[3] >> 1;
        if (N * Hp * Wp / 4 < net->wino_min_tiles) return false;
        return cg_conv2d_ups2_wino_supported((int)N, (int)Hp, (int)Wp, (int)m.ia[0], (int)m.ia[1], 5, 2) != 0;
    }
    static bool epilogue_ok(const Geo& g) {   // the skinny <= 4-plane 3x3 kernels cannot take a fused epilogue
        const bool skinny = g.ups == 0 && g.kH == 3 && g.kW == 3 && g.padH == 1 && g.padW == 1 && (g.Cout == 1 || g.Cout == 3) &&
                            (g.Cin == 64 || g.Cin == 128);
        return !skinny;
    }
    Prep prep_fwd(Mod& m, const Val& in) {
        Prep p;
        MS& s = S(m);
        if (m.kind == K_LINEAR) {
            Val x = in;
            const long o = m.ia[1];
            if (s.map_in && !(x.nd == 4 && x.fmt == NHWC && !x.ups && x.d[1] == s.mc && x.d[2] == s.mh && x.d[3] == s.mw)) s.map_in = false;
            if (s.map_in) {
                const long N = x.d[0];
                need_plain(m, true, s.mc, s.mh, s.mw);
                p.x = x; p.wsel = W_PLAIN_F; p.out = buf(m, "out", {N, o});
                p.g = Geo{(int)N, (int)s.mh, (int)s.mw, (int)s.mc, (int)o, (int)s.mh, (int)s.mw, 0, 0, 0};
                return p;
            }
            x = as_plain(x);
            const long N = x.d[0], i = x.numel() / x.d[0];
            need_plain(m, false);
            p.x = x; p.wsel = W_PLAIN_F; p.out = buf(m, "out", {N, o});
            p.g = Geo{(int)N, 1, 1, (int)i, (int)o, 1, 1, 0, 0, 0};
            return p;
        }
        Val x = as_nhwc(in, true);
        if (x.ups && !can_fold_ups(m)) x = materialise(x);
        const long N = x.d[0], H = x.d[2], W = x.d[3];
        const long Hp = H >> x.ups, Wp = W >> x.ups, Ho = H + 2 * m.padH() - m.kH() + 1, Wo = W + 2 * m.padW() - m.kW() + 1;
        if (x.d[1] != m.ia[0]) { err("cg_net: convolution %d got %ld input planes, expects %ld", m.id, x.d[1], m.ia[0]); }
        if (x.ups) { need_ups(m, false); p.wsel = W_PH_F; } else { need_plain(m, false); p.wsel = W_PLAIN_F; }
        p.x = x;
        p.out = buf(m, "out", {N, m.ia[1], Ho, Wo}, NHWC);
        p.g = Geo{(int)N, (int)Hp, (int)Wp, (int)m.ia[0], (int)m.ia[1], (int)m.kH(), (int)m.kW(), (int)m.padH(), (int)m.padW(), x.ups};
        return p;
    }
    // updateGradInput as a forward call on gradOutput with the backward-packed weights; ok == false: not this form (folded upsampling)
    Prep prep_gin(Mod& m, const Val& go) {
        Prep p;
        MS& s = S(m);
        if (m.kind == K_LINEAR) {
            Val dy = as_plain(go);
            const long N = dy.d[0], o = dy.numel() / dy.d[0], i = m.ia[0];
            p.x = dy;
            if (s.map_in) {   // dx comes out NHWC-flattened: wbT[co][(h*W+w)*C + c] (cg_pack_conv_weight_map)
                p.wsel = W_PLAIN_B; p.out = buf(m, "gin", {N, s.mc, s.mh, s.mw}, NHWC);
            } else {
                p.wsel = W_CANON; p.out = buf(m, "gin", {N, i});
            }
            p.g = Geo{(int)N, 1, 1, (int)o, (int)i, 1, 1, 0, 0, 0};
            return p;
        }
        const Val& x = s.x;
        if (x.ups) { p.ok = false; return p; }
        Val dy = as_nhwc(go);
        const long N = dy.d[0], Ho = dy.d[2], Wo = dy.d[3];
        p.x = dy; p.wsel = W_PLAIN_B;
        p.out = buf(m, "gin", {N, m.ia[0], x.d[2], x.d[3]}, NHWC);
        p.g = Geo{(int)N, (int)Ho, (int)Wo, (int)m.ia[1], (int)m.ia[0], (int)m.kH(), (int)m.kW(), (int)(m.kH() - 1 - m.padH()),
                  (int)(m.kW() - 1 - m.padW()), 0};
        return p;
    }
    struct PrepAcc { Val x, dy; Geo g; };
    PrepAcc prep_acc(Mod& m, const Val& go) {
        PrepAcc p;
        MS& s = S(m);
        p.x = s.x;
        if (m.kind == K_LINEAR) {
            p.dy = as_plain(go);
            if (s.map_in) p.g = Geo{(int)p.x.d[0], (int)s.mh, (int)s.mw, (int)s.mc, (int)m.ia[1], (int)s.mh, (int)s.mw, 0, 0, 0};
            else p.g = Geo{(int)p.x.d[0], 1, 1, (int)(p.x.numel() / p.x.d[0]), (int)m.ia[1], 1, 1, 0, 0, 0};
            return p;
        }
        p.dy = as_nhwc(go);
        const Val& x = s.x;
        p.g = Geo{(int)x.d[0], (int)(x.d[2] >> x.ups), (int)(x.d[3] >> x.ups), (int)m.ia[0], (int)m.ia[1], (int)m.kH(), (int)m.kW(),
                  (int)m.padH(), (int)m.padW(), x.ups};
        return p;
    }

    // ---------------------------------------------------------------------------------------- the GEMM launches of G conv / linear layers
    // Prepare the layers of 1..4 branches for ONE launch: every branch through `prep` (prep_fwd, or prep_gin with role "gin"); a real
    // group under option stacking gets outputs that are the slices of one block (seeded under `role`, then prepared again).  false: no
    // common launch - more than four branches, unequal geometry, a form `prep` refuses, a layer that takes Winograd, or (epilogue) one
    // that cannot carry an epilogue.
    bool prep_group(const vector<Mod*>& mods, const vector<Val>& ins, Prep (Compiler::*prep)(Mod&, const Val&), const char* role, bool epilogue,
                    vector<Prep>& preps) {
        const int G = (int)mods.size();
        for (int b = 0; b < G; ++b) preps.push_back((this->*prep)(*mods[b], ins[b]));
        bool ok = G <= 4, wino = false;
        for (int b = 0; b < G; ++b) {
            ok = ok && preps[b].ok && (!epilogue || epilogue_ok(preps[b].g));
            wino = wino || (ok && mods[b]->kind == K_CONV && preps[b].x.ups && use_wino(*mods[b], preps[b].x));
        }
        for (int b = 1; ok && b < G; ++b) ok = preps[b].g == preps[0].g;
        if (!ok || wino) return false;
        vector<Val> outs; for (auto& p : preps) outs.push_back(p.out);
        if (G > 1 && net->stacking && !stacked(outs, nullptr)) {
            seed_slices(mods, role, preps[0].out, preps[0].out.fmt);
            preps.clear();
            for (int b = 0; b < G; ++b) preps.push_back((this->*prep)(*mods[b], ins[b]));
        }
        return true;
    }
    // What a forward GEMM launch does behind the bias: nothing, the activations `acts` into `ya` (the pre-activation stays in the layer's
    // output, which the activation's backward needs), or the batch-norm statistics partials `part` of its output tile rows.
    struct Epi { vector<Mod*> acts; vector<Val> ya; Val part; };
    // One launch over the prepared layers: cg_conv2d_forward for a lone layer without an epilogue, _grouped for a group without one,
    // _ex otherwise.  bias false: the same launch as a data gradient (prep_gin), which adds none.
    void emit_gemm(const vector<Mod*>& mods, const vector<Prep>& preps, const Epi& e, bool bias = true) {
        const KTable* k = K();
        const int G = (int)mods.size();
        const Geo g = preps[0].g;
        ws_need(cg_conv2d_workspace_bytes_grouped(G, GEO(g)));
        if (e.acts.empty() && e.part.none) {
            if (G == 1) {
                const Prep p = preps[0]; Mod* mp = mods[0];
                emit([=](Run& c) { return k->conv2d_forward(c.CS(), c.P(p.x), wsel(mp, p.wsel), bias ? mp->b : nullptr, c.P(p.out), GEO(p.g), c.W(), c.WB()); });
                return;
            }
            emit([=](Run& c) {
                const float *x[4], *w[4], *bi[4]; float* y[4];
                for (int b = 0; b < G; ++b) { x[b] = c.P(preps[b].x); w[b] = wsel(mods[b], preps[b].wsel); bi[b] = mods[b]->b; y[b] = c.P(preps[b].out); }
                return k->conv2d_forward_grouped(c.CS(), G, x, w, bias ? bi : nullptr, y, GEO(g), c.W(), c.WB());
            });
            return;
        }
        const int code = e.acts.empty() ? 0 : e.acts[0]->kind == K_PRELU ? 1 : 2;
        const float slope = code == 2 ? e.acts[0]->fa[0] : 0.f;
        const vector<Mod*> ac = e.acts; const vector<Val> ys = e.ya; const Val part = e.part;
        emit([=](Run& c) {
            const float *x[4], *w[4], *bi[4], *al[4]; float *y[4], *ya[4];
            for (int b = 0; b < G; ++b) {
                x[b] = c.P(preps[b].x); w[b] = wsel(mods[b], preps[b].wsel); bi[b] = mods[b]->b; y[b] = c.P(preps[b].out);
                if (code) { al[b] = ac[b]->w; ya[b] = c.P(ys[b]); }
            }
            return k->conv2d_forward_ex(c.CS(), G, x, w, bi, y, GEO(g), code, slope, code == 1 ? al : nullptr, code ? ya : nullptr, c.P(part), c.W(), c.WB());
        });
    }
    vector<Val> fwd_gemm(const vector<Mod*>& mods, const vector<Prep>& preps, const Epi& e) {   // ... as the layers' forward
        emit_gemm(mods, preps, e);
        vector<Val> outs;
        for (size_t b = 0; b < mods.size(); ++b) {
            MS& s = S(*mods[b]);
            s.x = preps[b].x; s.out = preps[b].out; s.use_wino = false; s.use_wino22 = false;
            outs.push_back(preps[b].out);
        }
        return outs;
    }
    // Weight gradients of G >= 1 layers that share a geometry in one grouped launch.  Deferred (options defer_wgrad and fusion both on):
    // the split-K partials stay in the workspace slot `ws` (one per layer, grow-only) and are reduced by the next flush_wgrad on this
    // stream; else the launch reduces them itself in the stream's scratch.
    // (The fused localisation branch only runs with fusion on, so its four layers defer on the same predicate.)
    bool defer_wg() const { return net->defer_wgrad && net->fusion; }
    void emit_wgrad_group(const vector<Mod*>& mods, const vector<PrepAcc>& ap, void*& ws, size_t& ws_bytes) {
        const KTable* k = K();
        const int G = (int)mods.size();
        const Geo g = ap[0].g;
        const bool defer = defer_wg();
        const size_t need = std::max<size_t>(cg_conv2d_wgrad_workspace_bytes_grouped(G, GEO(g)), 4096);
        if (defer) {
            if (!dry && ws_bytes < need) { ws = alloc(need); ws_bytes = need; }
            if (!dry) pend[cs]++;
        } else ws_need(need);
        void* wsp = ws; const size_t wsb = ws_bytes;
        emit([=](Run& c) {
            const float *x[4], *d_[4]; float *gw[4], *gb[4];
            for (int b = 0; b < G; ++b) { x[b] = c.P(ap[b].x); d_[b] = c.P(ap[b].dy); gw[b] = mods[b]->gw; gb[b] = mods[b]->gb; }
            if (defer) return k->conv2d_wgrad_grouped_deferred(c.CS(), G, x, d_, gw, gb, GEO(g), c.scale, wsp, wsb);
            return k->conv2d_wgrad_grouped(c.CS(), G, x, d_, gw, gb, GEO(g), c.scale, c.W(), c.WB());
        });
    }

    // ---------------------------------------------------------------------------------------- forward of one module
    // One module with its own launches, drawing at `rng`; what they return is kept as the module's output.  nn.Sequential and
    // nn.ConcatTable are walked by gfwd alone (a lone module is a lockstep group of one).
    Val fwd(Mod& m, const Val& in) {
        Val out = fwd_launches(m, in);
        S(m).out = out;
        return out;
    }
    Val fwd_launches(Mod& m, const Val& in) {
        const KTable* k = K();
        MS& s = S(m);
        switch (m.kind) {
        case K_CONCAT: return fwd_concat(m, in);
        case K_LINEAR: case K_CONV: {
            if (m.kind == K_CONV) {
                Val x = as_nhwc(in, true);
                if (use_wino(m, x)) return fwd_wino(m, x, nullptr, nullptr);
            }
            vector<Prep> preps;
            prep_group({&m}, {in}, &Compiler::prep_fwd, "out", false, preps);   // a lone layer off the Winograd path: nothing to refuse
            return fwd_gemm({&m}, preps, Epi())[0];
        }
        case K_PRELU: {
            Val x = materialise(in);
            Val out = buf_like(m, "out", x, x.fmt);
            const long n = x.phys(); Mod* mp = &m;
            emit([=](Run& c) { return k->prelu_forward(c.CS(), c.P(x), mp->w, c.P(out), n); });
            s.x = x;
            return out;
        }
        case K_LRELU: {
            Val x = materialise(in);
            Val out = buf_like(m, "out", x, x.fmt);
            const long n = x.phys(); const float sl = m.fa[0];
            emit([=](Run& c) { return k->leakyrelu_forward(c.CS(), c.P(x), c.P(out), sl, n); });
            s.x = x;
            return out;
        }
        case K_SIGMOID: {
            Val x = materialise(in);
            Val out = buf_like(m, "out", x, x.fmt);
            const long n = x.phys();
            emit([=](Run& c) { return k->sigmoid_forward(c.CS(), c.P(x), c.P(out), n); });
            return out;
        }
        case K_BN: {
            Val x = as_nhwc(in);
            Val out;
            if (!m.train) {
                const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3], Mr = N * H * W;
                out = buf(m, "out", {N, C, H, W}, NHWC);
                Mod* mp = &m; const float eps = m.fa[0];
                emit([=](Run& c) { return k->bn_forward_eval(c.CS(), c.P(x), c.P(out), mp->w, mp->b, mp->rmean, mp->rvar, Mr, (int)C, eps); });
            } else {
                out = fwd_bn_train(m, nullptr, x, Stats());
            }
            s.x = x; s.bn_fused = false;
            return out;
        }
        case K_VIEW: {
            s.skip = false;
            Val x = as_plain(in);
            const long N = x.d[0];
            s.in_nd = x.nd; for (int i = 0; i < 4; ++i) s.in_shape[i] = x.d[i];
            Val out;
            if (m.ia[7] == 3) {
                const long C = m.ia[0], H = m.ia[1], W = m.ia[2];
                out = buf(m, "out", {N, C, H, W}, NHWC);
                emit([=](Run& c) { return k->nchw_to_nhwc(c.CS(), c.P(x), c.P(out), (int)N, (int)C, (int)H, (int)W); });
            } else {
                out = reshape(x, {N, m.ia[0]}, PLAIN);
            }
            return out;
        }
        case K_COPY: return in;
        case K_TRANSPOSE: {
            Val out;
            if (m.ia[0] == 0) {   // NCHW -> BHWD: with NHWC storage a relabeling of the same memory
                Val x = as_nhwc(in);
                out = reshape(x, {x.d[0], x.d[2], x.d[3], x.d[1]}, PLAIN, 0, true);
            } else {              // BHWD -> NCHW
                if (in.fmt != PLAIN) err("cg_net: nn.Transpose BHWD->NCHW expects a plain tensor");
                out = reshape(in, {in.d[0], in.d[3], in.d[1], in.d[2]}, NHWC, 0, true);
            }
            return out;
        }
        case K_UPS: {   // never materialised when a convolution consumes it
            Val x = as_nhwc(in);
            Val out = reshape(x, {x.d[0], x.d[1], 2 * x.d[2], 2 * x.d[3]}, NHWC, 1);
            return out;
        }
        case K_AVGPOOL: case K_MAXPOOL: {
            Val x = as_nhwc(in);
            const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
            Val out = buf(m, "out", {N, C, H / 2, W / 2}, NHWC);
            const bool mx = m.kind == K_MAXPOOL;
            emit([=](Run& c) { return (mx ? k->maxpool2_forward : k->avgpool2_forward)(c.CS(), c.P(x), c.P(out), (int)N, (int)H, (int)W, (int)C); });
            s.x = x;
            return out;
        }
        case K_SDROP: {
            Val x = as_nhwc(in);
            const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
            Val out = buf(m, "out", {N, C, H, W}, NHWC);
            const float p = m.fa[0];
            if (m.train) {
                Val noise = draw_masks(m, "noise", 1, N, C, &rng, false);
                emit([=](Run& c) { return k->mask_mul(c.CS(), c.P(x), c.P(noise), c.P(out), (int)N, H * W, (int)C, 1); });
                s.noise = noise;
            } else {
                emit_scaled_copy(out, x, 1.0f - p);
            }
            return out;
        }
        case K_DROP: {
            Val x = materialise(in);
            if (!m.train) return x;
            const long n = x.phys(); const float p = m.fa[0];
            Val noise = buf_like(m, "noise", x, x.fmt), out = buf_like(m, "out", x, x.fmt);
            const long off = rng; rng += n;
            emit([=](Run& c) { return k->rng_bernoulli_dev(c.CS(), c.P(noise), n, 1.0f - p, 1.0f / (1.0f - p), c.seed, c.roff + (uint64_t)off, c.rbase); });
            emit([=](Run& c) { return k->mask_mul(c.CS(), c.P(x), c.P(noise), c.P(out), 1, n, 1, 0); });
            s.noise = noise;
            return out;
        }
        case K_AFFMAT: {
            Val p = as_plain(in);
            const long N = p.d[0];
            Val out = buf(m, "out", {N, 2, 3});
            const int r = (int)m.ia[0], sc = (int)m.ia[1], tr = (int)m.ia[2];
            emit([=](Run& c) { return k->affine_matrix_forward(c.CS(), c.P(p), c.P(out), (int)N, r, sc, tr); });
            s.p = p;
            return out;
        }
        case K_AFFGRID: {
            const long N = in.d[0], H = m.ia[0], W = m.ia[1];
            Val out = buf(m, "out", {N, H, W, 2});
            Val T = in;
            emit([=](Run& c) { return k->affine_grid_forward(c.CS(), c.P(T), c.P(out), (int)N, (int)H, (int)W); });
            return out;
        }
        case K_SAMPLER: {
            if (!in.is_tab || in.tab.size() != 2) { err("cg_net: nn.BilinearSamplerBHWD expects {images, grids}"); return in; }
            Val img = in.tab[0], grid = in.tab[1];
            if (img.fmt != PLAIN || grid.fmt != PLAIN) err("cg_net: sampler inputs must be BHWD tensors");
            const long N = img.d[0], Hi = img.d[1], Wi = img.d[2], C = img.d[3], Ho = grid.d[1], Wo = grid.d[2];
            Val out = buf(m, "out", {N, Ho, Wo, C});
            emit([=](Run& c) { return k->bilinear_sampler_forward(c.CS(), c.P(img), c.P(grid), c.P(out), (int)N, (int)Hi, (int)Wi, (int)C, (int)Ho, (int)Wo); });
            s.in_img = img; s.in_grid = grid; s.has_shared = false;
            return out;
        }
        }
        err("cg_net: module kind %d has no forward", m.kind);
        return in;
    }
    // Batch-norm statistics partials a GEMM / Winograd epilogue left for the batch-norm behind the layer (rows 0: none, take cg_bn_stats)
    struct Stats { long rows = 0; Val part; };
    // upsample2 -> conv5x5 on the NHWC input x in Winograd F(2x2,3x3) (use_wino).  bn: the batch-norm (training) behind the layer - the
    // _stats entry point, whose epilogue writes that layer's statistics partials where the geometry allows (st)
    Val fwd_wino(Mod& m, const Val& x, Mod* bn, Stats* st) {
        const KTable* k = K();
        const long N = x.d[0], Hp = x.d[2] >> 1, Wp = x.d[3] >> 1, Ci = m.ia[0], Co = m.ia[1];
        need_ups(m, true);
        Val out = buf(m, "out", {N, Co, x.d[2], x.d[3]}, NHWC);
        Val v = buf(m, "wino_v", {(long)cg_conv2d_ups2_wino_v_floats((int)N, (int)Hp, (int)Wp, (int)Ci)});
        Mod* mp = &m;
        if (bn) {
            st->rows = (long)cg_conv2d_ups2_wino_stats_rows((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co);
            if (st->rows) st->part = buf(*bn, "stats_part", {st->rows, 2, Co});
            const Val part = st->part;
            emit([=](Run& c) { return k->conv2d_ups2_wino_forward_stats(c.CS(), c.P(x), mp->u_fwd, mp->b, c.P(out), c.P(v), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co,
                                                                       c.P(part)); });
        } else {
            emit([=](Run& c) { return k->conv2d_ups2_wino_forward(c.CS(), c.P(x), mp->u_fwd, mp->b, c.P(out), c.P(v), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co); });
        }
        MS& s = S(m);
        s.x = x; s.out = out; s.use_wino = true;
        return out;
    }
    // Training batch-norm of the NHWC tensor x: the statistics (st: finalised from an epilogue's partials), under sync-BN their exchange,
    // the global count, then normalise - with the PReLU `act` behind it in the same pass when given; the running statistics either
    // there or in cg_net_apply_running (bn_runs)
    Val fwd_bn_train(Mod& bn, Mod* act, const Val& x, const Stats& st) {
        const KTable* k = K();
        const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3], Mr = N * H * W;
        // (the module's own output before its sums, the activation's behind them: a trace names the exchanged buffer by allocation order)
        Val y = act ? Val() : buf(bn, "out", {N, C, H, W}, NHWC);
        Val sums = buf(bn, "sums", {2 * C}, PLAIN, 8), sm = buf(bn, "save_mean", {C}), sv = buf(bn, "save_std", {C});
        if (act) y = buf_like(*act, "out", x, NHWC);
        const long rows = st.rows; const Val part = st.part;
        if (rows) emit([=](Run& c) { return k->bn_stats_finalize(c.CS(), c.P(part), rows, (int)C, (double*)c.P(sums)); });
        else emit([=](Run& c) { return k->bn_stats(c.CS(), c.P(x), Mr, (int)C, (double*)c.P(sums)); });
        emit_allreduce_sum(sums, 2 * C, 1);
        const double cnt = (double)Mr * dp_factor();
        S(bn).count = cnt;
        Mod *bp = &bn, *ap = act; const float eps = bn.fa[0], mom = bn.fa[1];
        if (act)
            emit([=](Run& c) { const bool df = c.net->defer_running != 0;
                               return k->bn_act_forward(c.CS(), c.P(x), c.P(y), bp->w, bp->b, (const double*)c.P(sums), cnt, Mr, (int)C, eps, mom, df ? nullptr : bp->rmean,
                                                        df ? nullptr : bp->rvar, c.P(sm), c.P(sv), ap->w); });
        else
            emit([=](Run& c) { const bool df = c.net->defer_running != 0;
                               return k->bn_forward(c.CS(), c.P(x), c.P(y), bp->w, bp->b, (const double*)c.P(sums), cnt, Mr, (int)C, eps, mom,
                                                    df ? nullptr : bp->rmean, df ? nullptr : bp->rvar, c.P(sm), c.P(sv)); });
        if (!dry) pr->bn_runs.push_back({bp, sums, cnt, C, mom});
        return y;
    }
    // The [G * N, C] mask block `role` of G sibling nn.SpatialDropout modules (a lone one: G 1): branch b's [N, C] part is drawn at pos[b]
    // of the counter stream, which moves on by N * C.  one_launch: the G draws in one grouped launch instead of G launches.
    Val draw_masks(Mod& d0, const char* role, int G, long N, long C, long* pos, bool one_launch) {
        const KTable* k = K();
        Val mask = buf(d0, role, {G * N, C});
        const float p = d0.fa[0];
        long offs[4] = {0, 0, 0, 0};
        for (int b = 0; b < G; ++b) { offs[b] = pos[b]; pos[b] += N * C; }
        if (G > 1 && one_launch) {
            const long o0 = offs[0], o1 = offs[1], o2 = offs[2], o3 = offs[3];
            emit([=](Run& c) {
                // base-relative positions: the kernel adds *rbase to every one of them
                return k->rng_bernoulli_dev_grouped(c.CS(), c.P(mask), N * C, G, 1.0f - p, 1.0f, c.seed, c.roff + (uint64_t)o0, G > 1 ? c.roff + (uint64_t)o1 : 0,
                                                    G > 2 ? c.roff + (uint64_t)o2 : 0, G > 3 ? c.roff + (uint64_t)o3 : 0, c.rbase);
            });
            return mask;
        }
        for (int b = 0; b < G; ++b) {
            const long off = offs[b];
            Val nb = mask.at((size_t)b * N * C * 4);
            emit([=](Run& c) { return k->rng_bernoulli_dev(c.CS(), c.P(nb), N * C, 1.0f - p, 1.0f, c.seed, c.roff + (uint64_t)off, c.rbase); });
        }
        return mask;
    }

    // ---------------------------------------------------------------------------------------- lockstep forward of sibling modules
    static bool stackable(const Mod& m) {
        switch (m.kind) { case K_LRELU: case K_VIEW: case K_AVGPOOL: case K_MAXPOOL: case K_SDROP: case K_AFFMAT: case K_AFFGRID: return true; default: return false; }
    }
    // f(b) for every branch, each at its own position in the counter stream (`rng` while its launches are emitted)
    template <class F> vector<Val> per_branch(GCtx& ctx, F f) {
        vector<Val> outs;
        for (size_t b = 0; b < ctx.cur.size(); ++b) {
            const long saved = rng; rng = ctx.cur[b];
            outs.push_back(f((int)b));
            ctx.cur[b] = rng; rng = saved;
        }
        return outs;
    }
    vector<Val> gfwd_default(const vector<Mod*>& mods, const vector<Val>& ins, GCtx& ctx) {
        return per_branch(ctx, [&](int b) { return fwd(*mods[b], ins[b]); });
    }
    // a stacked tensor as G per-branch values / G per-branch values as one stacked tensor; a group of one is the tensor itself
    vector<Val> slices(const Val& Y, int G) { return G == 1 ? vector<Val>{Y} : split(Y, G); }
    Val gather(const Mod& owner, const vector<Val>& xs, const Val& like) {
        Val X;
        if (xs.size() == 1) return xs[0];
        return stacked(xs, &X) ? X : restack(owner, xs, like);
    }
    vector<Val> gfwd_stackable(const vector<Mod*>& mods, const vector<Val>& ins, GCtx& ctx) {
        Mod& m0 = *mods[0];
        Val X;
        if (!(net->stacking && stacked(ins, &X))) { S(m0).stk = 0; return gfwd_default(mods, ins, ctx); }
        vector<Val> ys = split(fwd(m0, X), (int)mods.size());
        S(m0).stk = ys[0].blk;
        for (size_t b = 0; b < mods.size(); ++b) S(*mods[b]).out = ys[b];
        return ys;
    }
    bool ran_stacked(Mod& m0) { MS& s = S(m0); return !s.out.none && !s.out.is_tab && s.out.blk && s.out.blk == s.stk; }

    vector<Val> gfwd(const vector<Mod*>& mods, const vector<Val>& ins, GCtx& ctx) {
        Mod& m0 = *mods[0];
        const KTable* k = K();
        const int G = (int)mods.size();
        // a group of one emits what the module emits on its own: the grouped / stacked / shared forms below are for real groups
        if (G == 1 && m0.kind != K_SEQ && m0.kind != K_CONCATTABLE) return gfwd_default(mods, ins, ctx);
        switch (m0.kind) {
        case K_SEQ: {
            // a localisation branch, or sibling ones on the SAME input (D32_st3's three transformers): one fused launch for the group
            // (fuse_locnet 2: ungrouped branches only)
            LocDesc ld;
            bool same = G <= 4 && (G == 1 || net->fuse_locnet != 2) && match_loc(m0, ins[0], ld);
            for (int b = 1; same && b < G; ++b) {
                LocDesc lb;
                same = ins[b].key() == ins[0].key() && ins[b].same_shape(ins[0]) && match_loc(*mods[b], ins[b], lb) && lb.S == ld.S && lb.Cin == ld.Cin &&
                       lb.P == ld.P && lb.ur == ld.ur && lb.us == ld.us && lb.ut == ld.ut && lb.slope == ld.slope;
            }
            if (same) return fwd_loc(mods, ins[0], ld);
            for (Mod* m : mods) S(*m).loc_fused = false;
            return gfwd_seq(mods, ins, ctx);
        }
        case K_CONCATTABLE: {
            const size_t nch = m0.kids.size();
            vector<vector<Val>> per_child;
            for (size_t j = 0; j < nch; ++j) {
                vector<Mod*> col; for (Mod* m : mods) col.push_back(&M(m->kids[j]));
                per_child.push_back(gfwd(col, ins, ctx));
            }
            vector<Val> outs;
            for (int b = 0; b < G; ++b) {
                Val t; t.is_tab = true; t.none = false;
                for (size_t j = 0; j < nch; ++j) t.tab.push_back(per_child[j][b]);
                S(*mods[b]).out = t;
                outs.push_back(t);
            }
            return outs;
        }
        case K_AVGPOOL: case K_MAXPOOL: {
            // sibling instances fed the SAME tensor (the localisation nets of D32_st3's three transformer branches all start by
            // pooling the trunk's output, models.lua:843) compute the same thing: one launch, shared result
            bool same = net->fusion && net->share_pool && !ins[0].is_tab;
            for (int b = 1; same && b < G; ++b) same = ins[b].key() == ins[0].key() && ins[b].same_shape(ins[0]) && ins[b].fmt == ins[0].fmt && ins[b].ups == ins[0].ups;
            if (same) {
                Val y = fwd(m0, ins[0]);
                for (Mod* m : mods) { S(*m).x = S(m0).x; S(*m).out = y; }
                S(m0).stk = 0; S(m0).shared_in = true;
                return vector<Val>(G, y);
            }
            S(m0).shared_in = false;
            return gfwd_stackable(mods, ins, ctx);
        }
        case K_SDROP: {
            // stacked form: every branch draws its own [N,C] mask at its own position of the counter stream (into one block),
            // then a single mask multiply runs over the stacked batch
            Val X;
            if (!(net->stacking && stacked(ins, &X))) { S(m0).stk = 0; return gfwd_default(mods, ins, ctx); }
            if (!m0.train) return gfwd_stackable(mods, ins, ctx);
            const long N = ins[0].d[0], C = ins[0].d[1], H = ins[0].d[2], W = ins[0].d[3];
            Val noise = draw_masks(m0, "noise.block", G, N, C, ctx.cur.data(), false);
            Val out = buf_like(m0, "out", X, NHWC);
            emit([=](Run& c) { return k->mask_mul(c.CS(), c.P(X), c.P(noise), c.P(out), (int)(G * N), H * W, (int)C, 1); });
            vector<Val> ys = split(out, G), ns = split(noise, G);
            S(m0).stk = ys[0].blk; S(m0).noise_block = noise;
            for (int b = 0; b < G; ++b) { S(*mods[b]).out = ys[b]; S(*mods[b]).noise = ns[b]; }
            return ys;
        }
        case K_LINEAR: case K_CONV: {
            vector<Prep> preps;
            if (!prep_group(mods, ins, &Compiler::prep_fwd, "out", false, preps)) return gfwd_default(mods, ins, ctx);
            return fwd_gemm(mods, preps, Epi());
        }
        case K_PRELU: {
            bool ok = net->stacking;
            for (auto& x : ins) ok = ok && !x.is_tab && !x.ups;
            if (ok) seed_slices(mods, "out", ins[0], ins[0].fmt);
            return gfwd_default(mods, ins, ctx);
        }
        case K_SAMPLER: {
            // sibling transformers sampling the SAME image tensor with stacked grids (D32_st3's branches): one launch over the
            // G*N samples; else one launch per branch into the slices of one block
            MS& s0 = S(m0);
            s0.has_shared = false;
            if (net->stacking) {
                const Val &img = ins[0].tab[0], &gr0 = ins[0].tab[1];
                const long N = img.d[0], Hi = img.d[1], Wi = img.d[2], C = img.d[3], Ho = gr0.d[1], Wo = gr0.d[2];
                vector<Val> grids; for (auto& i_ : ins) grids.push_back(i_.tab[1]);
                Val GR;
                bool sh = net->fusion && net->sampler_shared && stacked(grids, &GR) && img.fmt == PLAIN && GR.fmt == PLAIN;
                for (auto& i_ : ins) sh = sh && i_.tab[0].key() == img.key() && i_.tab[0].same_shape(img);
                if (sh) {
                    Val out = buf(m0, "out.block", {G * N, Ho, Wo, C});
                    emit([=](Run& c) { return k->bilinear_sampler_forward_shared(c.CS(), G, c.P(img), c.P(GR), c.P(out), (int)N, (int)Hi, (int)Wi, (int)C, (int)Ho, (int)Wo); });
                    vector<Val> ys = split(out, G);
                    for (int b = 0; b < G; ++b) { S(*mods[b]).out = ys[b]; S(*mods[b]).in_img = ins[b].tab[0]; S(*mods[b]).in_grid = ins[b].tab[1]; }
                    s0.has_shared = true; s0.shared_out = out; s0.shared_grids = GR;
                    return ys;
                }
                Val shp = mkval(nullptr, {N, Ho, Wo, C});
                seed_slices(mods, "out", shp, PLAIN);
            }
            return gfwd_default(mods, ins, ctx);
        }
        default:
            if (stackable(m0)) return gfwd_stackable(mods, ins, ctx);
            return gfwd_default(mods, ins, ctx);
        }
    }

    // ---------------------------------------------------------------------------------------- nn.Sequential: segments
    vector<Seg> plan(const Mod& q) {
        vector<Seg> out;
        const int n = (int)q.kids.size();
        int i = 0;
        while (i < n) {
            Mod& m = M(q.kids[i]);
            int kind = S_ONE, j = i + 1;
            if (net->fusion) {
                Mod* nx = i + 1 < n ? &M(q.kids[i + 1]) : nullptr;
                Mod* nx2 = i + 2 < n ? &M(q.kids[i + 2]) : nullptr;
                Mod* nx3 = i + 3 < n ? &M(q.kids[i + 3]) : nullptr;
                if (m.kind == K_CONV && nx && nx->kind == K_BN && nx->train && nx2 && nx2->kind == K_PRELU) { kind = S_GEMM_BN_ACT; j = i + 3; }
                else if (m.is_gemm() && nx && nx->is_act() && !(nx2 && nx2->is_pool())) { kind = S_GEMM_ACT; j = i + 2; }
                else if (m.kind == K_VIEW && m.ia[7] == 1 && nx && nx->kind == K_LINEAR && net->view_fuse) {
                    if (nx2 && nx2->is_act() && !(nx3 && nx3->is_pool())) { kind = S_VIEW_GEMM_ACT; j = i + 3; }
                    else { kind = S_VIEW_GEMM; j = i + 2; }
                } else if (m.is_act() && nx && nx->is_pool()) {
                    const bool drop = nx2 && nx2->kind == K_SDROP && nx2->train;
                    kind = S_ACT_POOL; j = i + (drop ? 3 : 2);
                } else if (net->head_fuse && net->cat_fuse && m.kind == K_CONCAT && nx && nx->kind == K_SDROP && nx->train) {
                    kind = S_CAT_DROP; j = i + 2;
                } else if (net->head_fuse && m.kind == K_DROP && m.train && nx && nx->kind == K_LINEAR && nx->ia[1] <= 4 && nx2 && nx2->kind == K_SIGMOID) {
                    kind = S_HEAD; j = i + 3;
                }
            }
            out.push_back(Seg{kind, i, j});
            i = j;
        }
        return out;
    }
    vector<Val> gfwd_seq(const vector<Mod*>& qs, const vector<Val>& ins, GCtx& ctx) {
        vector<Val> cur = ins;
        vector<Seg> pl = plan(*qs[0]);
        for (Mod* q : qs) { S(*q).ran = pl; S(*q).ran_set = true; }
        auto col = [&](int t) { vector<Mod*> c; for (Mod* q : qs) c.push_back(&M(q->kids[t])); return c; };
        auto kid = [&](int b, int t) -> Mod& { return M(qs[b]->kids[t]); };
        for (const Seg& sg : pl) {
            const int i = sg.i;
            switch (sg.kind) {
            case S_ONE: cur = gfwd(col(i), cur, ctx); break;
            case S_GEMM_ACT: cur = fwd_gemm_act(col(i), col(i + 1), cur, ctx); break;
            case S_ACT_POOL: cur = fwd_act_pool(col(i), col(i + 1), sg.j - i == 3 ? col(i + 2) : vector<Mod*>{}, cur, ctx); break;
            case S_VIEW_GEMM: cur = fwd_view_gemm(col(i), col(i + 1), {}, cur, ctx); break;
            case S_VIEW_GEMM_ACT: cur = fwd_view_gemm(col(i), col(i + 1), col(i + 2), cur, ctx); break;
            // no lockstep form: the fused segment branch after branch
            case S_CAT_DROP: cur = per_branch(ctx, [&](int b) { return fwd_concat(kid(b, i), cur[b], &kid(b, i + 1)); }); break;
            case S_HEAD: cur = per_branch(ctx, [&](int b) { return fwd_head(kid(b, i), kid(b, i + 1), kid(b, i + 2), cur[b]); }); break;
            default: cur = per_branch(ctx, [&](int b) { return fwd_gemm_bn_act(kid(b, i), kid(b, i + 1), kid(b, i + 2), cur[b]); }); break;
            }
            if (failed) break;
        }
        for (size_t b = 0; b < qs.size(); ++b) S(*qs[b]).out = cur[b];
        return cur;
    }

    // [conv|linear, PReLU|LeakyReLU] x G branches: one (grouped) GEMM launch whose epilogue writes the pre-activation (what the
    // activation's backward needs) and the activation
    vector<Val> fwd_gemm_act(const vector<Mod*>& convs, const vector<Mod*>& acts, const vector<Val>& xs, GCtx& ctx) {
        const int G = (int)convs.size();
        vector<Prep> preps;
        if (!prep_group(convs, xs, &Compiler::prep_fwd, "out", true, preps)) return gfwd(acts, gfwd(convs, xs, ctx), ctx);
        if (G > 1 && net->stacking) seed_slices(acts, "out", preps[0].out, preps[0].out.fmt);
        vector<Val> ys;
        for (int b = 0; b < G; ++b) ys.push_back(buf_like(*acts[b], "out", preps[b].out, preps[b].out.fmt));
        vector<Val> po = fwd_gemm(convs, preps, Epi{acts, ys, Val()});
        for (int b = 0; b < G; ++b) { MS& sa = S(*acts[b]); sa.x = po[b]; sa.out = ys[b]; }
        if (G > 1 && stackable(*acts[0])) {   // let the parameter-free activation run its backward as one stacked launch
            Val Xs, Ys;
            if (stacked(po, &Xs) && stacked(ys, &Ys)) { S(*acts[0]).x = Xs; S(*acts[0]).stk = ys[0].blk; }
            else S(*acts[0]).stk = 0;
        }
        return ys;
    }

    // [View(C*H*W), Linear, (activation)] x G branches (models.lua:696-698, 849-851): the linear layer consumes the NHWC map
    vector<Val> fwd_view_gemm(const vector<Mod*>& views, const vector<Mod*>& lins, const vector<Mod*>& acts, vector<Val> xs, GCtx& ctx) {
        const int G = (int)views.size();
        const Val& x0 = xs[0];
        bool ok = !x0.is_tab && x0.nd == 4 && x0.fmt == NHWC && !x0.ups;
        long C = 0, H = 0, W = 0;
        if (ok) {
            C = x0.d[1]; H = x0.d[2]; W = x0.d[3];
            ok = H * W <= 64 && C % 16 == 0 && views[0]->ia[0] == C * H * W && lins[0]->ia[0] == C * H * W;
            for (auto& x : xs) ok = ok && !x.is_tab && x.same_shape(x0) && x.fmt == NHWC && !x.ups;
        }
        for (int b = 0; b < G; ++b) {
            S(*views[b]).skip = ok;
            MS& sl = S(*lins[b]); sl.map_in = ok; sl.mc = C; sl.mh = H; sl.mw = W;
        }
        if (ok) {
            for (int b = 0; b < G; ++b) { MS& sv = S(*views[b]); sv.out = Val(); sv.in_nd = 4; for (int i = 0; i < 4; ++i) sv.in_shape[i] = xs[b].d[i]; }
        } else {
            xs = gfwd(views, xs, ctx);
        }
        if (!acts.empty()) return fwd_gemm_act(lins, acts, xs, ctx);
        return gfwd(lins, xs, ctx);
    }

    // [PReLU|LeakyReLU, Pool 2x2, (SpatialDropout, training)] x G branches in one pass over the stacked input
    vector<Val> fwd_act_pool(const vector<Mod*>& acts, const vector<Mod*>& pools, const vector<Mod*>& drops, const vector<Val>& xs, GCtx& ctx) {
        const KTable* k = K();
        const int G = (int)acts.size();
        Mod &a0 = *acts[0], &p0 = *pools[0];
        Mod* d0 = drops.empty() ? nullptr : drops[0];
        const Val& x0 = xs[0];
        Val X; bool haveX = false;
        long N = 0, C = 0, H = 0, W = 0;
        if (!x0.is_tab && x0.nd == 4 && x0.fmt == NHWC && !x0.ups && G <= 4) {
            N = x0.d[0]; C = x0.d[1]; H = x0.d[2]; W = x0.d[3];
            if (C % 4 == 0 && H % 2 == 0 && W % 2 == 0) {
                if (G == 1) { X = x0; haveX = true; }
                else haveX = net->stacking && stacked(xs, &X);
            }
        }
        if (!haveX) {   // the separate modules
            S(a0).fused = false;
            vector<vector<Mod*>> chain = {acts, pools};
            if (!drops.empty()) chain.push_back(drops);
            vector<Val> cur = xs;
            for (auto& colm : chain) cur = gfwd(colm, cur, ctx);
            return cur;
        }
        const int code = a0.kind == K_PRELU ? 1 : 2;
        const float slope = code == 1 ? 0.f : a0.fa[0];
        Mod& last = d0 ? *d0 : p0;
        Val out = buf(last, "out.fused", {G * N, C, H / 2, W / 2}, NHWC);
        Val mask; bool have_mask = false;
        if (d0) { mask = draw_masks(*d0, "noise.block", G, N, C, ctx.cur.data(), true); have_mask = true; }
        const int pool_max = p0.kind == K_MAXPOOL ? 1 : 0;
        vector<Mod*> ac = acts;
        emit([=](Run& c) {
            const float* al[4];
            for (int b = 0; b < G; ++b) al[b] = ac[b]->w;
            return k->act_pool2_mask_forward(c.CS(), c.P(X), c.P(out), have_mask ? c.P(mask) : nullptr, G, (int)N, (int)H, (int)W, (int)C, code, slope,
                                             code == 1 ? al : nullptr, pool_max);
        });
        vector<Val> outs = slices(out, G), masks;
        if (have_mask) masks = slices(mask, G);
        for (int b = 0; b < G; ++b) {
            MS& sa = S(*acts[b]); sa.x = xs[b]; sa.out = Val();
            MS& sp = S(*pools[b]); sp.x = Val(); sp.out = d0 ? Val() : outs[b];
            if (d0) { MS& sd = S(*drops[b]); sd.noise = masks[b]; sd.out = outs[b]; }
        }
        MS& s0 = S(a0);
        s0.fused = true; s0.fG = G; s0.fX = X; s0.fmask = have_mask ? mask : Val(); s0.fN = N; s0.fC = C; s0.fH = H; s0.fW = W;
        return outs;
    }

    // [conv, SpatialBatchNormalization (training), PReLU] (models.lua:206-208, 212-214, 218-220): batch statistics from the GEMM /
    // Winograd epilogue, normalise + activate in one pass; the normalised tensor is not kept (the backward recomputes it)
    Val fwd_gemm_bn_act(Mod& conv, Mod& bn, Mod& act, const Val& in) {
        const KTable* k = K();
        Val x = as_nhwc(in, true);
        const long C = conv.ia[1];
        if (C % 4 != 0) { S(bn).bn_fused = false; return fwd(act, fwd(bn, fwd(conv, in))); }
        Stats st; Val out;
        Mod* cp = &conv;
        if (use_wino(conv, x)) {
            out = fwd_wino(conv, x, &bn, &st);
        } else if (use_wino22(conv, x)) {
            // forward in F(2x2,2x2); the layer's state is that of the phase-folded direct path, which its backward takes
            Prep p = prep_fwd(conv, x);
            const long N = x.d[0], Hp = x.d[2] >> 1, Wp = x.d[3] >> 1, Ci = conv.ia[0];
            if (!dry && !conv.u22) {
                conv.u22 = (float*)alloc(cg_conv2d_ups2_wino22_u_floats((int)Ci, (int)C) * 4);
                conv.u22b = (float*)alloc(cg_conv2d_ups2_wino22_u_floats((int)Ci, (int)C) * 4);
                conv.dirty_ups = true;
            }
            out = p.out;
            Val v = buf(conv, "wino22_v", {(long)cg_conv2d_ups2_wino22_v_floats((int)N, (int)Hp, (int)Wp, (int)Ci)});
            st.rows = (long)cg_conv2d_ups2_wino_stats_rows((int)N, (int)Hp, (int)Wp, (int)Ci, (int)C);
            if (st.rows) st.part = buf(bn, "stats_part", {st.rows, 2, C});
            const Val px = p.x, part = st.part;
            emit([=](Run& c) { return k->conv2d_ups2_wino22_forward_stats(c.CS(), c.P(px), cp->u22, cp->b, c.P(out), c.P(v), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)C,
                                                                         c.P(part)); });
            S(conv).x = p.x; S(conv).out = p.out; S(conv).use_wino = false; S(conv).use_wino22 = true;
        } else {
            vector<Prep> preps;
            prep_group({&conv}, {x}, &Compiler::prep_fwd, "out", false, preps);   // a lone layer off the Winograd path: nothing to refuse
            st.rows = epilogue_ok(preps[0].g) ? (long)cg_conv2d_stats_rows(GEO(preps[0].g)) : 0;
            if (st.rows) st.part = buf(bn, "stats_part", {st.rows, 2, C});
            out = fwd_gemm({&conv}, preps, Epi{{}, {}, st.part})[0];
        }
        Val y = fwd_bn_train(bn, &act, out, st);
        const long Mr = out.d[0] * out.d[2] * out.d[3];
        MS& sb = S(bn); sb.x = out; sb.out = Val(); sb.bn_fused = true; sb.bnM = Mr; sb.bnC = C;
        MS& sa = S(act); sa.x = Val(); sa.out = y;
        return y;
    }

    // ---------------------------------------------------------------------------------------- fused localisation branch
    // nn.Sequential{ localisation net (models.lua:842-855), AffineTransformMatrixGenerator, AffineGridGeneratorBHWD } (:874-879) as
    // cg_locnet_forward / cg_locnet_backward: one launch each way instead of ~10 / ~12, off the GEMM path (csrc/locnet.hip).
    struct LocDesc { Mod *conv1, *conv2, *lin1, *lin2; int S, Cin, P, ur, us, ut, Hg, Wg; float slope; };
    bool match_loc(Mod& q, const Val& in, LocDesc& d) {
        if (!net->fuse_locnet || !net->fusion || q.kind != K_SEQ || q.kids.size() != 3) return false;
        Mod& L = M(q.kids[0]);
        static const int want[10] = {K_AVGPOOL, K_CONV, K_LRELU, K_CONV, K_LRELU, K_AVGPOOL, K_VIEW, K_LINEAR, K_LRELU, K_LINEAR};
        if (L.kind != K_SEQ || L.kids.size() != 10 || M(q.kids[1]).kind != K_AFFMAT || M(q.kids[2]).kind != K_AFFGRID) return false;
        for (int i = 0; i < 10; ++i) if (M(L.kids[i]).kind != want[i]) return false;
        if (in.is_tab || in.none || in.nd != 4 || in.fmt != NHWC || in.ups || in.d[2] != in.d[3] || in.d[2] % 4) return false;
        d.conv1 = &M(L.kids[1]); d.conv2 = &M(L.kids[3]); d.lin1 = &M(L.kids[7]); d.lin2 = &M(L.kids[9]);
        d.S = (int)(in.d[2] / 2); d.Cin = (int)in.d[1]; d.P = (int)d.lin2->ia[1];
        auto conv_ok = [](const Mod& c, long ci) { return c.ia[0] == ci && c.ia[1] == 16 && c.kW() == 3 && c.kH() == 3 && c.padW() == 1 && c.padH() == 1; };
        if (!conv_ok(*d.conv1, d.Cin) || !conv_ok(*d.conv2, 16)) return false;
        const long K3 = 16L * (d.S / 2) * (d.S / 2);
        if (M(L.kids[6]).ia[7] != 1 || M(L.kids[6]).ia[0] != K3 || d.lin1->ia[0] != K3 || d.lin1->ia[1] != 64 || d.lin2->ia[0] != 64) return false;
        d.slope = M(L.kids[2]).fa[0];
        if (M(L.kids[4]).fa[0] != d.slope || M(L.kids[8]).fa[0] != d.slope) return false;
        if (!(d.slope > 0.f)) return false;   // cg_locnet_backward reads LeakyReLU's side off the stored activations: slope > 0 only
        const Mod &am = M(q.kids[1]), &ag = M(q.kids[2]);
        d.ur = (int)am.ia[0]; d.us = (int)am.ia[1]; d.ut = (int)am.ia[2]; d.Hg = (int)ag.ia[0]; d.Wg = (int)ag.ia[1];
        if (d.P != d.ur + d.us + 2 * d.ut) return false;
        return cg_locnet_supported(d.S, d.Cin, d.P) != 0;
    }
    static void loc_weights(const vector<Mod*>& qs, Net* n, const float* w[48]) {
        for (size_t b = 0; b < qs.size(); ++b) {
            const Mod& L = *n->mods[qs[b]->kids[0]];
            const Mod *c1 = n->mods[L.kids[1]].get(), *c2 = n->mods[L.kids[3]].get(), *l1 = n->mods[L.kids[7]].get(), *l2 = n->mods[L.kids[9]].get();
            const float* v[12] = {c1->w, c1->b, c2->w, c2->b, l1->w, l1->b, l2->w, l2->b, c1->wf, c1->wb, c2->wf, c2->wb};
            for (int k = 0; k < 12; ++k) w[12 * b + k] = v[k];
        }
    }
    vector<Val> fwd_loc(const vector<Mod*>& qs, const Val& in, const LocDesc& d) {
        const KTable* k = K();
        const int G = (int)qs.size();
        Mod& q0 = *qs[0];
        const long N = in.d[0], S_ = d.S, Cin = d.Cin, K3 = 16L * (S_ / 2) * (S_ / 2);
        Val pooled = buf(q0, "loc.pooled", {G * N, Cin, S_, S_}, NHWC), h1 = buf(q0, "loc.h1", {G * N, 16, S_, S_}, NHWC),
            m2 = buf(q0, "loc.m2", {G * N, 16, S_, S_}, NHWC), h2 = buf(q0, "loc.h2", {G * N, K3}), h3 = buf(q0, "loc.h3", {G * N, 64}),
            prm = buf(q0, "loc.params", {G * N, d.P}), grid = buf(q0, "loc.grid", {G * N, d.Hg, d.Wg, 2});
        for (Mod* q : qs) {   // the two convolutions' packed copies (refreshed with every other layer's after a parameter update)
            const Mod& L = M(q->kids[0]);
            need_plain(M(L.kids[1]), false); need_plain(M(L.kids[3]), false);
        }
        Net* n_ = net; vector<Mod*> qv = qs; const LocDesc dd = d; Val x = in;
        emit([=](Run& c) {
            const float* w[48];
            loc_weights(qv, n_, w);
            return k->locnet_forward(c.CS(), G, (int)N, c.P(x), 1, w, dd.S, dd.Cin, dd.P, dd.ur, dd.us, dd.ut, dd.slope, dd.Hg, dd.Wg, c.P(pooled), c.P(h1),
                                     c.P(m2), c.P(h2), c.P(h3), c.P(prm), c.P(grid));
        });
        vector<Val> outs = slices(grid, G);
        for (int b = 0; b < G; ++b) {
            MS& s = S(*qs[b]);
            s.out = outs[b]; s.loc_fused = true; s.locG = G; s.locN = N;
            s.ran_set = false;
        }
        MS& s0 = S(q0);
        s0.x = in;
        return outs;
    }
    vector<Val> bwd_loc(const vector<Mod*>& qs, const vector<Val>& gouts, bool acc) {
        const KTable* k = K();
        const int G = (int)qs.size();
        Mod& q0 = *qs[0];
        MS& s0 = S(q0);
        LocDesc d;
        if (!match_loc(q0, s0.x, d)) { err("cg_net: fused localisation branch lost its shape"); return gouts; }
        const long N = s0.locN, S_ = d.S, Cin = d.Cin, K3 = 16L * (S_ / 2) * (S_ / 2);
        Val GG = gather(q0, gouts, gouts[0]);
        Val pooled = buf(q0, "loc.pooled", {G * N, Cin, S_, S_}, NHWC), h1 = buf(q0, "loc.h1", {G * N, 16, S_, S_}, NHWC),
            m2 = buf(q0, "loc.m2", {G * N, 16, S_, S_}, NHWC), h2 = buf(q0, "loc.h2", {G * N, K3}), h3 = buf(q0, "loc.h3", {G * N, 64}),
            prm = buf(q0, "loc.params", {G * N, d.P});
        Val ga1 = buf(q0, "loc.ga1", {G * N, 16, S_, S_}, NHWC), ga2 = buf(q0, "loc.ga2", {G * N, 16, S_, S_}, NHWC), g3 = buf(q0, "loc.g3", {G * N, 64}),
            g4 = buf(q0, "loc.g4", {G * N, d.P}), gx = buf(q0, "loc.gx", {G * N, Cin, 2 * S_, 2 * S_}, NHWC);
        Net* n_ = net; vector<Mod*> qv = qs; const LocDesc dd = d;
        emit([=](Run& c) {
            const float* w[48];
            loc_weights(qv, n_, w);
            return k->locnet_backward(c.CS(), G, (int)N, w, dd.S, dd.Cin, dd.P, dd.ur, dd.us, dd.ut, dd.slope, dd.Hg, dd.Wg, c.P(h1), c.P(m2), c.P(h3), c.P(prm),
                                      c.P(GG), c.P(ga1), c.P(ga2), c.P(g3), c.P(g4), c.P(gx));
        });
        if (acc) {
            // weight gradients of the four layers on the GEMM path (grouped over the sibling branches), reductions deferred; their
            // gradOutputs come out of the launch above, so the fork sits behind it
            wg_fork();
            const long P_ = d.P;
            MS* s0p = &s0;
            wg_after_dgrad([this, G, N, S_, Cin, K3, P_, pooled, ga1, h1, ga2, h2, g3, h3, g4, qv, s0p]() {
            struct W { int li; Val x, dy; Geo g; };
            const W ws_[4] = {
                {1, pooled, ga1, Geo{(int)N, (int)S_, (int)S_, (int)Cin, 16, 3, 3, 1, 1, 0}},
                {3, h1, ga2, Geo{(int)N, (int)S_, (int)S_, 16, 16, 3, 3, 1, 1, 0}},
                {7, h2, g3, Geo{(int)N, 1, 1, (int)K3, 64, 1, 1, 0, 0, 0}},
                {9, h3, g4, Geo{(int)N, 1, 1, 64, (int)P_, 1, 1, 0, 0, 0}}};
            for (int wi = 0; wi < 4; ++wi) {
                const W& wv = ws_[wi];
                const size_t xs = (size_t)wv.x.phys() / G * 4, ds = (size_t)wv.dy.phys() / G * 4;
                vector<Mod*> lay; vector<PrepAcc> ap;   // branch b: its layer, its part of the stacked activations / gradients
                for (int b = 0; b < G; ++b) {
                    lay.push_back(&M(M(qv[b]->kids[0]).kids[wv.li]));
                    ap.push_back(PrepAcc{wv.x.at(b * xs), wv.dy.at(b * ds), wv.g});
                }
                emit_wgrad_group(lay, ap, s0p->loc_ws[wi], s0p->loc_ws_bytes[wi]);
            }
            });
        }
        return share_gin(qs, gx);
    }

    // ---------------------------------------------------------------------------------------- nn.Concat(2)
    std::string signature(const Mod& m) {   // two modules with equal signatures run the same launches with the same geometry
        std::string s = "(" + std::to_string(m.kind);
        for (int i = 0; i < 8; ++i) s += "," + std::to_string(m.ia[i]);
        char b[64]; snprintf(b, sizeof b, ",%a,%a,%d", m.fa[0], m.fa[1], m.train); s += b;
        for (int c : m.kids) s += signature(M(c));
        return s + ")";
    }
    vector<vector<int>> branch_groups(const Mod& q) {   // option grouped 0: every branch a group of its own
        vector<std::pair<std::string, vector<int>>> by;
        for (size_t i = 0; i < q.kids.size(); ++i) {
            std::string sg = signature(M(q.kids[i]));
            bool found = false;
            for (auto& e : by) if (net->grouped && e.first == sg) { e.second.push_back((int)i); found = true; break; }
            if (!found) by.push_back({sg, {(int)i}});
        }
        vector<vector<int>> groups;
        for (auto& e : by)
            for (size_t k0 = 0; k0 < e.second.size(); k0 += 4) groups.emplace_back(e.second.begin() + k0, e.second.begin() + std::min(k0 + 4, e.second.size()));
        std::sort(groups.begin(), groups.end(), [](const vector<int>& a, const vector<int>& b) { return a[0] < b[0]; });
        return groups;
    }
    // thunks[0] on the current stream, the others forked onto side streams and joined (D32_st3: the long chain of launch-bound
    // kernels of the three transformer branches hides under the big GEMMs of the two-convolution branch)
    void run_groups(const vector<std::function<void()>>& thunks) {
        const bool multi = net->grouped && net->overlap_groups && thunks.size() > 1 && cs == 0 && thunks.size() <= 4;
        if (!multi) { for (auto& f : thunks) f(); return; }
        emit_event(EV_RECORD, EV_FORK, 0);
        for (size_t t = 1; t < thunks.size(); ++t) {
            const int sidx = (int)t;
            use_stream(sidx);
            cs = sidx;
            emit_event(EV_WAIT, EV_FORK, 0);
            thunks[t]();
            flush_wgrad();
            emit_event(EV_RECORD, EV_JOIN, sidx);
            cs = 0;
        }
        thunks[0]();
        for (size_t t = 1; t < thunks.size(); ++t) emit_event(EV_WAIT, EV_JOIN, (int)t);
    }
    // Record / wait for an event of the net on the CURRENT stream; in trace mode the line event|<record|wait>|<name>|s<stream index>.
    // The event is looked up when the op runs (ensure_streams creates them after the plan is compiled): fork_ev, side_ev[k - 1] ("join<k>"),
    // wg_fork_ev[k] ("wgfork<k>"), wg_join_ev[k] ("wgjoin<k>").
    enum { EV_RECORD = 0, EV_WAIT = 1 };
    enum { EV_FORK = 0, EV_JOIN, EV_WGFORK, EV_WGJOIN };
    void emit_event(int what, int kind, int k) {
        static const char* const names[] = {"fork", "join", "wgfork", "wgjoin"};
        const int s = cs;
        const std::string line = std::string(what == EV_RECORD ? "event|record|" : "event|wait|") + names[kind] + (kind == EV_FORK ? "" : std::to_string(k)) +
                                 "|s" + std::to_string(s);
        emit([=](Run& c) {
            Net* n = c.net;
            if (n->trace) { trace_note(n, line); return 0; }
            const hipEvent_t e = kind == EV_FORK ? n->fork_ev : kind == EV_JOIN ? n->side_ev[k - 1] : kind == EV_WGFORK ? n->wg_fork_ev[k] : n->wg_join_ev[k];
            const hipStream_t st = (hipStream_t)c.S(s);
            return (what == EV_RECORD ? hipEventRecord(e, st) : hipStreamWaitEvent(st, e, 0)) == hipSuccess ? 0 : 1;
        });
    }
    void flush_wgrad() {   // reduce the weight-gradient partials queued on the CURRENT stream in one launch
        if (dry || !pend[cs]) return;
        const KTable* k = K();
        emit([=](Run& c) { return k->conv2d_wgrad_flush(c.CS()); });
        pend[cs] = 0;
    }
    // ---- weight gradients beside the data-gradient chain (option wgrad_stream).  accGradParameters of a layer reads the layer's saved
    // input and its gradOutput, and nothing before the optimiser step (or the layer's gradient bucket) reads what it writes; the data
    // gradient is what every layer in front of it waits for.  So in Module:backward the weight-gradient launches (GEMM, partial
    // reductions, the Winograd-domain path, the localisation nets' four) go to stream 4 + s, forked from stream s at the point where
    // gradOutput is complete, and are joined into stream 0 once, at the end of the pass.  The launch-bound kernels between two data
    // gradients (BN backward sums, activation / pooling backward, sampler and localisation backward) then run under a GEMM instead of
    // alone on the chip (profiles/r04_wgrad_stream_ab.txt).
    bool wg_on() const { return net->wgrad_stream && net->fusion && acc_pass && !dry && cs < 4; }
    void wg_fork() {   // call on stream s where the gradOutput the weight gradient reads is complete
        if (!wg_on()) return;
        emit_event(EV_RECORD, EV_WGFORK, cs);
    }
    int wg_enter() {   // later launches go to the weight-gradient stream; returns the stream index to hand back to wg_leave
        const int s = cs;
        if (!wg_on()) return s;
        use_stream(4 + s);
        cs = 4 + s;
        emit_event(EV_WAIT, EV_WGFORK, s);
        wg_used[s] = true; wg_unjoined[s] = true;
        return s;
    }
    void wg_leave(int s) { cs = s; }
    void wg_before_dgrad() { wg_fork(); }                                      // call in front of a layer's data-gradient launch ...
    void wg_after_dgrad(std::function<void()> f) {                             // ... and behind it, with the layer's weight-gradient launches
        const int s_ = wg_enter(); f(); wg_leave(s_);
    }
    void wg_join_all() {   // end of the pass: reductions still queued on the weight-gradient streams, then stream 0 waits for them
        if (dry) return;
        const int back = cs;
        for (int s = 0; s < 4; ++s) {
            if (!wg_used[s]) continue;
            cs = 4 + s;
            flush_wgrad();
            emit_event(EV_RECORD, EV_WGJOIN, s);
            cs = 0;
            emit_event(EV_WAIT, EV_WGJOIN, s);
            wg_used[s] = false;
        }
        cs = back;
    }
    long count_draws(Mod& m, const Val& in) {   // counter-stream draws of one forward of `m` (no launches, no state kept)
        Prog tmp; tmp.net = net;
        Prog* save = pr;
        pr = &tmp; ++dry;
        GCtx ctx{{0}};
        gfwd({&m}, {in}, ctx);
        --dry; pr = save;
        return ctx.cur[0];
    }
    // drop: the nn.SpatialDropout (training) right behind this nn.Concat in its Sequential, to run inside the concat launch
    Val fwd_concat(Mod& q, const Val& in, Mod* drop = nullptr) {
        const KTable* k = K();
        const int nb = (int)q.kids.size();
        vector<Val> outs(nb);
        // every branch draws where a branch-after-branch walk would, whatever order (and stream) the groups are emitted in
        vector<long> base(nb);
        for (int i = 0; i < nb; ++i) { base[i] = rng; rng += count_draws(M(q.kids[i]), in); }
        vector<std::function<void()>> thunks;
        for (auto& idxs : branch_groups(q)) {
            thunks.push_back([&, idxs]() {
                GCtx ctx; vector<Mod*> mods; vector<Val> ins;
                for (int i : idxs) { ctx.cur.push_back(base[i]); mods.push_back(&M(q.kids[i])); ins.push_back(in); }
                vector<Val> res = gfwd(mods, ins, ctx);
                for (size_t t = 0; t < idxs.size(); ++t) outs[idxs[t]] = as_nhwc(res[t]);
            });
        }
        run_groups(thunks);
        const long N = outs[0].d[0], H = outs[0].d[2], W = outs[0].d[3];
        MS& s = S(q);
        s.sizes.clear();
        long Ct = 0; bool all4 = true;
        for (auto& o : outs) { s.sizes.push_back(o.d[1]); Ct += o.d[1]; all4 = all4 && o.d[1] % 4 == 0; }
        Val out = buf(q, "out", {N, Ct, H, W}, NHWC);
        s.cat_drop = false;
        if (drop && net->fusion && net->cat_fuse && nb <= 4 && all4) {   // concat and the dropout behind it in one launch
            vector<long> sz = s.sizes;
            MS& sd = S(*drop);
            Val noise = buf(*drop, "noise", {N, Ct});
            const long off = rng; rng += N * Ct;
            const float pdrop = drop->fa[0];
            emit([=](Run& c) {
                const float* src[4]; int cc[4];
                for (int i = 0; i < nb; ++i) { src[i] = c.P(outs[i]); cc[i] = (int)sz[i]; }
                return k->concat_channels_dropout(c.CS(), nb, src, cc, c.P(out), c.P(noise), (int)N, H * W, 1.0f - pdrop, 1.0f, c.seed, c.roff + (uint64_t)off, c.rbase);
            });
            s.cat_drop = true;
            s.out = Val();            // the undropped concatenation is never stored
            sd.noise = noise; sd.out = out;
            return out;
        }
        if (net->fusion && net->cat_fuse && nb <= 4 && all4) {   // one launch for all branches
            vector<long> sz = s.sizes;
            emit([=](Run& c) {
                const float* src[4]; int cc[4];
                for (int i = 0; i < nb; ++i) { src[i] = c.P(outs[i]); cc[i] = (int)sz[i]; }
                return k->concat_channels(c.CS(), nb, src, cc, c.P(out), N * H * W);
            });
        } else {
            long off = 0;
            for (int i = 0; i < nb; ++i) {
                const long ci = s.sizes[i], o_ = off; Val src = outs[i];
                emit([=](Run& c) { return k->copy_channels(c.CS(), c.P(src), c.P(out), N * H * W, (int)ci, 0, (int)Ct, (int)o_, (int)ci); });
                off += ci;
            }
        }
        s.out = out;
        if (drop) return fwd(*drop, out);
        return out;
    }
    Val bwd_concat(Mod& q, const Val& in, const Val& go_, bool acc, Mod* drop = nullptr) {
        const KTable* k = K();
        const int nb = (int)q.kids.size();
        MS& s = S(q);
        const bool masked = drop && s.cat_drop;                 // the split launch multiplies by the dropout mask
        Val go = go_;
        if (drop && !masked) go = bwd(*drop, s.out, go_, acc);   // the forward ran the two modules separately
        // channel slices of the gradient, one per branch; the slices of a lockstep group are the parts of one block
        Val g = as_nhwc(go);
        const long N = g.d[0], Ct = g.d[1], H = g.d[2], W = g.d[3];
        vector<Val> dst(nb); vector<bool> have(nb, false);
        vector<vector<int>> groups = branch_groups(q);
        if (net->stacking) {
            for (auto& idxs : groups) {
                bool eq = idxs.size() > 1;
                for (int i : idxs) eq = eq && s.sizes[i] == s.sizes[idxs[0]];
                if (!eq) continue;
                Val block = buf(q, "gslice_block" + std::to_string(idxs[0]), {(long)idxs.size() * N, s.sizes[idxs[0]], H, W}, NHWC);
                vector<Val> sl = split(block, (int)idxs.size());
                for (size_t t = 0; t < idxs.size(); ++t) { dst[idxs[t]] = sl[t]; have[idxs[t]] = true; }
            }
        }
        bool all4 = true;
        for (int i = 0; i < nb; ++i) {
            if (!have[i]) dst[i] = buf(q, "gslice" + std::to_string(i), {N, s.sizes[i], H, W}, NHWC);
            all4 = all4 && s.sizes[i] % 4 == 0;
        }
        if (masked) {
            vector<long> sz = s.sizes;
            Val noise = S(*drop).noise;
            emit([=](Run& c) {
                float* d_[4]; int cc[4];
                for (int i = 0; i < nb; ++i) { d_[i] = c.P(dst[i]); cc[i] = (int)sz[i]; }
                return k->split_channels_masked(c.CS(), nb, c.P(g), c.P(noise), d_, cc, (int)N, H * W);
            });
            S(*drop).gin = Val();
        } else if (net->fusion && net->cat_fuse && nb <= 4 && all4) {
            vector<long> sz = s.sizes;
            emit([=](Run& c) {
                float* d_[4]; int cc[4];
                for (int i = 0; i < nb; ++i) { d_[i] = c.P(dst[i]); cc[i] = (int)sz[i]; }
                return k->split_channels(c.CS(), nb, c.P(g), d_, cc, N * H * W);
            });
        } else {
            long off = 0;
            for (int i = 0; i < nb; ++i) {
                const long ci = s.sizes[i], o_ = off; Val d_ = dst[i];
                emit([=](Run& c) { return k->copy_channels(c.CS(), c.P(g), c.P(d_), N * H * W, (int)Ct, (int)o_, (int)ci, 0, (int)ci); });
                off += ci;
            }
        }
        vector<Val> grads(nb);
        vector<std::function<void()>> thunks;
        for (auto& idxs : groups) {
            thunks.push_back([&, idxs]() {
                vector<Mod*> mods; vector<Val> ins, gs;
                for (int i : idxs) { mods.push_back(&M(q.kids[i])); ins.push_back(in); gs.push_back(dst[i]); }
                vector<Val> res = gbwd(mods, ins, gs, acc);
                for (size_t t = 0; t < idxs.size(); ++t) grads[idxs[t]] = as_nhwc(res[t]);
            });
        }
        run_groups(thunks);
        // gradInput = ((g0 + g1) + g2) + g3
        Val accv = buf_like(q, "gsum", grads[0], NHWC);
        const long n = accv.phys();
        if (net->fusion && net->cat_fuse && nb >= 2 && nb <= 4 && grads[0].phys() % 4 == 0) {
            emit([=](Run& c) {
                const float* src[4];
                for (int i = 0; i < nb; ++i) src[i] = c.P(grads[i]);
                return k->sum_n(c.CS(), nb, src, c.P(accv), n);
            });
        } else {
            Val g0 = grads[0];
            emit([=](Run& c) { return k->memcpy_d2d(c.CS(), c.P(accv), c.P(g0), (size_t)n * 4); });
            for (int i = 1; i < nb; ++i) { Val gi = grads[i]; emit([=](Run& c) { return k->axpy(c.CS(), 1.0f, c.P(gi), c.P(accv), n); }); }
        }
        s.gin = accv;
        return accv;
    }

    // [nn.Dropout (training), nn.Linear(F, O <= 4), nn.Sigmoid]: the discriminator's head (models.lua:699-701) as one launch each way
    Val fwd_head(Mod& drop, Mod& lin, Mod& sig, const Val& in) {
        const KTable* k = K();
        Val x = as_plain(in);
        const long N = x.d[0], F = lin.ia[0], O = lin.ia[1];
        MS &sd = S(drop), &sl = S(lin), &ss = S(sig);
        sd.head_fused = false;
        if (x.nd != 2 || x.d[1] != F || !cg_drop_linear_sigmoid_supported((int)N, (int)F, (int)O)) {
            Val a = fwd(drop, in);
            Val b = fwd(lin, a);
            return fwd(sig, b);
        }
        Val noise = buf_like(drop, "noise", x, PLAIN), xd = buf_like(drop, "out", x, PLAIN);
        Val z = buf(lin, "out", {N, O}), p = buf(sig, "out", {N, O});
        const long off = rng; rng += N * F;
        const float pdrop = drop.fa[0];
        Mod* lp = &lin;
        emit([=](Run& c) {
            if (!lp->w) return cg::fail("cg_net: layer %d has no weight bound (cg_net_bind)", lp->id);
            return k->drop_linear_sigmoid_forward(c.CS(), c.P(x), lp->w, lp->b, c.P(noise), c.P(xd), c.P(z), c.P(p), (int)N, (int)F, (int)O, 1.0f - pdrop,
                                                  1.0f / (1.0f - pdrop), c.seed, c.roff + (uint64_t)off, c.rbase);
        });
        sd.head_fused = true; sd.noise = noise; sd.out = xd; sd.x = x;
        sl.x = xd; sl.out = z; sl.map_in = false;
        ss.out = p;
        return p;
    }
    Val bwd_head(Mod& drop, Mod& lin, Mod& sig, const Val& go, bool acc) {
        const KTable* k = K();
        MS &sd = S(drop), &sl = S(lin), &ss = S(sig);
        Val g = as_plain(go);
        const long N = sd.x.d[0], F = lin.ia[0], O = lin.ia[1];
        Val gi = buf_like(drop, "gin", sd.x, PLAIN);
        Val p = ss.out, xd = sd.out, noise = sd.noise;
        Mod* lp = &lin;
        emit([=](Run& c) {
            return k->drop_linear_sigmoid_backward(c.CS(), c.P(g), c.P(p), c.P(xd), c.P(noise), lp->w, c.P(gi), acc ? lp->gw : nullptr, acc ? lp->gb : nullptr,
                                                   (int)N, (int)F, (int)O, acc ? c.scale : 0.f);
        });
        ss.gin = Val(); sl.gin = Val(); sd.gin = gi;
        return gi;
    }

    // ---------------------------------------------------------------------------------------- backward of one module
    // acc: Module:backward (gradInput + accGradParameters, scaled by Run::scale), else updateGradInput only.
    void wgrad(Mod& m, const Val& go) {   // accGradParameters of a conv / linear layer
        const KTable* k = K();
        MS& s = S(m);
        Mod* mp = &m;
        if (m.kind == K_CONV && s.x.ups && s.use_wino) {
            // Winograd-domain weight gradient from the transformed input the forward of this batch left in wino_v
            Val dy = as_nhwc(go);
            const Val& x = s.x;
            const long N = x.d[0], Hp = x.d[2] >> 1, Wp = x.d[3] >> 1, Ci = m.ia[0], Co = m.ia[1];
            Val v = buf(m, "wino_v", {(long)cg_conv2d_ups2_wino_v_floats((int)N, (int)Hp, (int)Wp, (int)Ci)});
            ws_need(cg_conv2d_ups2_wino_wgrad_workspace_bytes((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co));
            emit([=](Run& c) { return k->conv2d_ups2_wino_wgrad(c.CS(), c.P(v), c.P(dy), mp->gw, mp->gb, (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co, c.scale, c.W(), c.WB()); });
            return;
        }
        PrepAcc p = prep_acc(m, go);
        if (defer_wg()) return emit_wgrad_group({&m}, {p}, s.wg_ws, s.wg_ws_bytes);
        ws_need(cg_conv2d_wgrad_workspace_bytes(GEO(p.g)));   // a lone layer that reduces at once: the plain entry point
        emit([=](Run& c) { return k->conv2d_wgrad(c.CS(), c.P(p.x), c.P(p.dy), mp->gw, mp->gb, GEO(p.g), c.scale, c.W(), c.WB()); });
    }
    Val dgrad(Mod& m, const Val& go) {    // updateGradInput of a conv / linear layer
        const KTable* k = K();
        MS& s = S(m);
        Mod* mp = &m;
        if (m.kind == K_CONV && s.x.ups) {
            // gradient w.r.t. the low-res tensor behind the virtual upsampling (its 2x2 block sum folded in); handed to
            // nn.SpatialUpSamplingNearest as the dual of its lazy output: shape = logical, ups = 1
            Val dy = as_nhwc(go);
            const Val& x = s.x;
            const long N = dy.d[0], Hl = x.d[2], Wl = x.d[3], Hp = Hl >> 1, Wp = Wl >> 1, Ci = m.ia[0], Co = m.ia[1];
            Val lo = buf(m, "gin_lo", {N, Ci, Hp, Wp}, NHWC);
            const int kk = (int)m.kH(), pad = (int)m.padH();
            if (s.use_wino) {
                Val vdy = buf(m, "wino_vdy", {(long)cg_conv2d_ups2_wino_v_floats((int)N, (int)Hp, (int)Wp, (int)(4 * Co))});
                const long np = net->wino_dsplit ? (long)cg_conv2d_ups2_wino_dgrad_part_floats((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co) : 0;
                if (np) {
                    Val part = buf(m, "wino_dpart", {np});
                    emit([=](Run& c) { return k->conv2d_ups2_wino_dgrad_split(c.CS(), c.P(dy), mp->u_bwd, c.P(lo), c.P(vdy), c.P(part), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co); });
                } else
                    emit([=](Run& c) { return k->conv2d_ups2_wino_dgrad(c.CS(), c.P(dy), mp->u_bwd, c.P(lo), c.P(vdy), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co); });
            } else if (s.use_wino22 && (net->wino22 & 2) && mp->u22b && cg_conv2d_ups2_wino22_dgrad_supported((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co)) {
                Val vdy = buf(m, "wino22_vdy", {(long)cg_conv2d_ups2_wino22_dgrad_v_floats((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co)});
                emit([=](Run& c) { return k->conv2d_ups2_wino22_dgrad(c.CS(), c.P(dy), mp->u22b, c.P(lo), c.P(vdy), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co); });
            } else {
                ws_need(cg_conv2d_dgrad_ups2_workspace_bytes((int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co, kk, pad));
                emit([=](Run& c) { return k->conv2d_dgrad_ups2(c.CS(), c.P(dy), mp->wb_ph, c.P(lo), (int)N, (int)Hp, (int)Wp, (int)Ci, (int)Co, kk, pad, c.W(), c.WB()); });
            }
            Val gi = reshape(lo, {N, Ci, Hl, Wl}, NHWC, 1);
            s.gin = gi;
            return gi;
        }
        Prep p = prep_gin(m, go);
        emit_gemm({&m}, {p}, Epi(), false);
        s.gin = p.out;
        return p.out;
    }
    // The `count` local sums `bs` of a batch-norm backward as what the normalisation's backward reads beside them: themselves, or under
    // sync-BN their sum over the ranks in a second buffer (`role`)
    Val bn_sums_all(Mod& bn, const Val& bs, const char* role, long count) {
        if (!(net->world > 1 && net->sync_bn)) return bs;
        const KTable* k = K();
        Val gs = buf(bn, role, {count}, PLAIN, 8);
        emit([=](Run& c) { return k->memcpy_d2d(c.CS(), c.P(gs), c.P(bs), (size_t)count * 8); });
        emit_allreduce_sum(gs, count, 1);
        return gs;
    }
    Val bwd(Mod& m, const Val& in, const Val& go, bool acc) {   // one module's launches; what they return is kept as its gradInput
        Val gi = bwd_launches(m, in, go, acc);
        S(m).gin = gi;
        return gi;
    }
    Val bwd_launches(Mod& m, const Val& in, const Val& go, bool acc) {
        const KTable* k = K();
        MS& s = S(m);
        Mod* mp = &m;
        switch (m.kind) {
        case K_CONCAT: return bwd_concat(m, in, go, acc);
        case K_LINEAR: case K_CONV: {
            if (acc) wg_before_dgrad();
            Val gi = dgrad(m, go);
            if (acc) { Mod* mp_ = &m; const Val go_ = go; wg_after_dgrad([this, mp_, go_]() { wgrad(*mp_, go_); }); }
            return gi;
        }
        case K_PRELU: {
            const Val& x = s.x;
            Val dy = match_fmt(go, x);
            Val gi = buf_like(m, "gin", x, x.fmt);
            const long n = x.phys();
            if (acc) ws_need(cg_prelu_backward_workspace_bytes(n));
            emit([=](Run& c) { return k->prelu_backward(c.CS(), c.P(x), c.P(dy), mp->w, c.P(gi), acc ? mp->gw : nullptr, acc ? c.scale : 0.f, n,
                                                        acc ? c.W() : nullptr, acc ? c.WB() : 0); });
            return gi;
        }
        case K_LRELU: {
            const Val& x = s.x;
            Val dy = match_fmt(go, x);
            Val gi = buf_like(m, "gin", x, x.fmt);
            const long n = x.phys(); const float sl = m.fa[0];
            emit([=](Run& c) { return k->leakyrelu_backward(c.CS(), c.P(x), c.P(dy), c.P(gi), sl, n); });
            return gi;
        }
        case K_SIGMOID: {
            const Val& y = s.out;
            Val dy = match_fmt(go, y);
            Val gi = buf_like(m, "gin", y, y.fmt);
            const long n = y.phys();
            emit([=](Run& c) { return k->sigmoid_backward(c.CS(), c.P(y), c.P(dy), c.P(gi), n); });
            return gi;
        }
        case K_BN: {
            if (!m.train) { err("cg_net: batch-norm backward in evaluate() mode is not on the path"); return go; }
            const Val& x = s.x;
            Val dy = as_nhwc(go);
            const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3], Mr = N * H * W;
            Val bs = buf(m, "bsums", {2 * C}, PLAIN, 8), sm = buf(m, "save_mean", {C}), sv = buf(m, "save_std", {C});
            emit([=](Run& c) { return k->bn_backward_stats(c.CS(), c.P(x), c.P(dy), c.P(sm), c.P(sv), Mr, (int)C, (double*)c.P(bs)); });
            Val gs = bn_sums_all(m, bs, "bsums_g", 2 * C);
            Val gi = buf_like(m, "gin", x, NHWC);
            const double cnt = s.count;
            emit([=](Run& c) { return k->bn_backward(c.CS(), c.P(x), c.P(dy), mp->w, c.P(sm), c.P(sv), (const double*)c.P(gs), cnt, (const double*)c.P(bs), Mr, (int)C,
                                                     c.P(gi), acc ? mp->gw : nullptr, acc ? mp->gb : nullptr, acc ? c.scale : 0.f); });
            return gi;
        }
        case K_VIEW: {
            if (s.skip) return go;   // fused into the nn.Linear behind it, whose gradInput already is the NHWC map
            Val g = as_plain(go);
            Val gi = g; gi.nd = s.in_nd; for (int i = 0; i < 4; ++i) gi.d[i] = s.in_shape[i];
            gi.fmt = PLAIN; gi.blk = 0; gi.gi = gi.gc = 0;
            return gi;
        }
        case K_COPY: return go;
        case K_TRANSPOSE: {
            Val gi;
            if (m.ia[0] == 0) {   // forward was NCHW -> BHWD: relabel the BHWD gradient as the NHWC-stored NCHW one
                if (go.fmt != PLAIN) err("cg_net: nn.Transpose backward expects a BHWD tensor");
                gi = reshape(go, {go.d[0], go.d[3], go.d[1], go.d[2]}, NHWC, 0, true);
            } else {
                Val g = as_nhwc(go);
                gi = reshape(g, {g.d[0], g.d[2], g.d[3], g.d[1]}, PLAIN, 0, true);
            }
            return gi;
        }
        case K_UPS: {
            Val gi;
            if (go.fmt == NHWC && go.ups) {   // the consumer conv already folded the 2x2 block sum
                gi = reshape(go, {go.d[0], go.d[1], go.d[2] / 2, go.d[3] / 2}, NHWC, 0);
            } else {
                Val g = as_nhwc(go);
                const long N = g.d[0], C = g.d[1], H2 = g.d[2], W2 = g.d[3];
                gi = buf(m, "gin", {N, C, H2 / 2, W2 / 2}, NHWC);
                emit([=](Run& c) { return k->upsample2x_backward(c.CS(), c.P(g), c.P(gi), (int)N, (int)(H2 / 2), (int)(W2 / 2), (int)C); });
            }
            return gi;
        }
        case K_AVGPOOL: case K_MAXPOOL: {
            const Val& x = s.x;
            Val g = as_nhwc(go);
            const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
            Val gi = buf_like(m, "gin", x, NHWC);
            if (m.kind == K_AVGPOOL) emit([=](Run& c) { return k->avgpool2_backward(c.CS(), c.P(g), c.P(gi), (int)N, (int)H, (int)W, (int)C); });
            else emit([=](Run& c) { return k->maxpool2_backward(c.CS(), c.P(x), c.P(g), c.P(gi), (int)N, (int)H, (int)W, (int)C); });
            return gi;
        }
        case K_SDROP: {
            Val g = as_nhwc(go);
            const long N = g.d[0], C = g.d[1], H = g.d[2], W = g.d[3];
            Val gi = buf_like(m, "gin", g, NHWC);
            if (m.train) {
                Val noise = s.noise;
                emit([=](Run& c) { return k->mask_mul(c.CS(), c.P(g), c.P(noise), c.P(gi), (int)N, H * W, (int)C, 1); });
            } else {
                emit_scaled_copy(gi, g, 1.0f - m.fa[0]);
            }
            return gi;
        }
        case K_DROP: {
            if (!m.train) return go;
            Val g = go;
            Val gi = buf_like(m, "gin", g, g.fmt);
            Val noise = s.noise; const long n = g.phys();
            emit([=](Run& c) { return k->mask_mul(c.CS(), c.P(g), c.P(noise), c.P(gi), 1, n, 1, 0); });
            return gi;
        }
        case K_AFFMAT: {
            const Val& p = s.p;
            Val gi = buf_like(m, "gin", p, PLAIN);
            const long N = p.d[0]; const int r = (int)m.ia[0], sc = (int)m.ia[1], tr = (int)m.ia[2];
            Val g = go;
            emit([=](Run& c) { return k->affine_matrix_backward(c.CS(), c.P(p), c.P(g), c.P(gi), (int)N, r, sc, tr); });
            return gi;
        }
        case K_AFFGRID: {
            const long N = go.d[0], H = m.ia[0], W = m.ia[1];
            Val gi = buf(m, "gin", {N, 2, 3});
            Val g = go;
            emit([=](Run& c) { return k->affine_grid_backward(c.CS(), c.P(g), c.P(gi), (int)N, (int)H, (int)W); });
            return gi;
        }
        case K_SAMPLER: {
            const Val &img = s.in_img, &grid = s.in_grid;
            const long N = img.d[0], Hi = img.d[1], Wi = img.d[2], C = img.d[3], Ho = grid.d[1], Wo = grid.d[2];
            if (go.fmt != PLAIN) err("cg_net: sampler gradOutput must be a BHWD tensor");
            Val gimg = buf_like(m, "gimg", img, PLAIN), ggrid = buf_like(m, "ggrid", grid, PLAIN);
            Val g = go;
            emit([=](Run& c) { return k->bilinear_sampler_backward(c.CS(), c.P(img), c.P(grid), c.P(g), c.P(gimg), c.P(ggrid), (int)N, (int)Hi, (int)Wi, (int)C, (int)Ho, (int)Wo); });
            Val t; t.is_tab = true; t.none = false; t.tab = {gimg, ggrid};
            return t;
        }
        }
        err("cg_net: module kind %d has no backward", m.kind);
        return go;
    }
    Val table_sum(Mod& owner, const vector<Val>& grads) {   // nn.ConcatTable: gradInput = sum of the branches' gradInputs
        const KTable* k = K();
        Val accv; bool have = false;
        for (const Val& g : grads) {
            if (g.none) continue;
            if (!have) { accv = g; have = true; continue; }
            Val a = accv.nd == 4 ? as_nhwc(accv) : accv, b = g.nd == 4 ? as_nhwc(g) : g;
            Val out = buf_like(owner, "sum", a, a.fmt);
            const long n = a.phys();
            emit([=](Run& c) { return k->add(c.CS(), c.P(a), c.P(b), c.P(out), n); });
            accv = out;
        }
        S(owner).gin = accv;
        return accv;
    }

    // ---------------------------------------------------------------------------------------- nn.Sequential backward
    // root: the net's own nn.Sequential, whose gradient buckets are complete segment by segment
    vector<Val> gbwd_seq(const vector<Mod*>& qs, const vector<Val>& ins, const vector<Val>& gouts, bool acc, bool root) {
        vector<Val> cur = gouts;
        const int G = (int)qs.size();
        MS& s0 = S(*qs[0]);
        vector<Seg> pl = s0.ran;
        if (!s0.ran_set) for (int t = 0; t < (int)qs[0]->kids.size(); ++t) pl.push_back(Seg{S_ONE, t, t + 1});
        auto col = [&](int t) { vector<Mod*> c; for (Mod* q : qs) c.push_back(&M(q->kids[t])); return c; };
        auto kid = [&](int b, int t) -> Mod& { return M(qs[b]->kids[t]); };
        for (int si = (int)pl.size() - 1; si >= 0; --si) {
            const Seg& sg = pl[si];
            const int i = sg.i;
            vector<Val> inp;
            if (i == 0) inp = ins; else for (int b = 0; b < G; ++b) inp.push_back(S(kid(b, i - 1)).out);
            auto drops = [&](int b0, int b1) {   // the SpatialDropouts of an [activation, pool, dropout] segment, branches [b0, b1)
                vector<Mod*> c; for (int b = b0; b < b1 && sg.j - i == 3; ++b) c.push_back(&kid(b, i + 2)); return c;
            };
            // what the forward left says how the segment ran: as one lockstep launch, as a fused launch per branch, or module by module
            bool own = true;
            for (int b = 0; b < G; ++b) {
                switch (sg.kind) {
                case S_ACT_POOL: own = own && S(kid(b, i)).fused && S(kid(b, i)).fG == 1; break;
                case S_GEMM_BN_ACT: own = own && S(kid(b, i + 1)).bn_fused; break;
                case S_CAT_DROP: break;   // bwd_concat takes the dropout behind it either way
                case S_HEAD: own = own && S(kid(b, i)).head_fused; break;
                default: own = false; break;
                }
            }
            if (sg.kind == S_ACT_POOL && S(kid(0, i)).fused && S(kid(0, i)).fG == G) {
                cur = bwd_act_pool(col(i), col(i + 1), drops(0, G), cur, acc);
            } else if (own) {
                for (int b = 0; b < G; ++b) {
                    switch (sg.kind) {
                    case S_ACT_POOL: cur[b] = bwd_act_pool({&kid(b, i)}, {&kid(b, i + 1)}, drops(b, b + 1), {cur[b]}, acc)[0]; break;
                    case S_GEMM_BN_ACT: cur[b] = bwd_gemm_bn_act(kid(b, i), kid(b, i + 1), kid(b, i + 2), inp[b], cur[b], acc); break;
                    case S_CAT_DROP: cur[b] = bwd_concat(kid(b, i), inp[b], cur[b], acc, &kid(b, i + 1)); break;
                    default: cur[b] = bwd_head(kid(b, i), kid(b, i + 1), kid(b, i + 2), cur[b], acc); break;
                    }
                }
            } else {   // S_ONE, S_GEMM_ACT (both outputs exist), or a chain whose forward ran unfused
                for (int t = sg.j - 1; t >= i; --t) {
                    vector<Val> mi;
                    if (t == i) mi = inp; else for (int b = 0; b < G; ++b) mi.push_back(S(kid(b, t - 1)).out);
                    cur = gbwd(col(t), mi, cur, acc);
                }
            }
            if (root && acc) bucket_done(i);
            if (failed) break;
        }
        for (int b = 0; b < G; ++b) S(*qs[b]).gin = cur[b];
        return cur;
    }

    // ---------------------------------------------------------------------------------------- lockstep backward of sibling modules
    vector<Val> gbwd_default(const vector<Mod*>& mods, const vector<Val>& ins, const vector<Val>& gouts, bool acc) {
        vector<Val> out;
        for (size_t b = 0; b < mods.size(); ++b) out.push_back(bwd(*mods[b], ins[b], gouts[b], acc));
        return out;
    }
    vector<Val> share_gin(const vector<Mod*>& mods, const Val& block) {   // a stacked gradInput as the siblings' gradInputs, its parts
        vector<Val> gs = slices(block, (int)mods.size());
        for (size_t b = 0; b < mods.size(); ++b) S(*mods[b]).gin = gs[b];
        return gs;
    }
    vector<Val> gbwd_stackable(const vector<Mod*>& mods, const vector<Val>& ins, const vector<Val>& gouts, bool acc) {
        Mod& m0 = *mods[0];
        if (!ran_stacked(m0)) return gbwd_default(mods, ins, gouts, acc);
        Val X;
        stacked(ins, &X);
        Val Gd = gather(m0, gouts, (!S(m0).out.none && !S(m0).out.is_tab) ? S(m0).out : gouts[0]);
        return share_gin(mods, bwd(m0, X, Gd, false));
    }
    vector<Val> gbwd(const vector<Mod*>& mods, const vector<Val>& ins, const vector<Val>& gouts, bool acc, bool root = false) {
        Mod& m0 = *mods[0];
        const KTable* k = K();
        const int G = (int)mods.size();
        if (G == 1 && m0.kind != K_SEQ && m0.kind != K_CONCATTABLE) return gbwd_default(mods, ins, gouts, acc);   // as in gfwd
        switch (m0.kind) {
        case K_SEQ:
            if (S(m0).loc_fused && S(m0).locG == G) return bwd_loc(mods, gouts, acc);
            return gbwd_seq(mods, ins, gouts, acc, root);
        case K_CONCATTABLE: {
            const size_t nch = m0.kids.size();
            vector<vector<Val>> per_child;
            for (size_t j = 0; j < nch; ++j) {
                vector<Mod*> col; vector<Val> gj;
                for (int b = 0; b < G; ++b) { col.push_back(&M(mods[b]->kids[j])); gj.push_back(gouts[b].tab[j]); }
                per_child.push_back(gbwd(col, ins, gj, acc));
            }
            vector<Val> blocks; bool all = net->stacking && G > 1;
            for (auto& c_ : per_child) {
                Val B;
                bool tens = true; for (auto& t : c_) tens = tens && !t.none && !t.is_tab;
                if (all && tens && stacked(c_, &B)) blocks.push_back(B); else all = false;
            }
            if (all) {   // one add per pair of children over the stacked batch
                return share_gin(mods, table_sum(m0, blocks));
            }
            vector<Val> outs;
            for (int b = 0; b < G; ++b) {
                vector<Val> gs; for (size_t j = 0; j < nch; ++j) gs.push_back(per_child[j][b]);
                outs.push_back(table_sum(*mods[b], gs));
            }
            return outs;
        }
        case K_AVGPOOL: case K_MAXPOOL: {
            MS& s0 = S(m0);
            if (s0.shared_in && m0.kind == K_AVGPOOL) {
                vector<Val> gs; for (auto& g : gouts) gs.push_back(as_nhwc(g));
                Val Gd;
                if (stacked(gs, &Gd)) {   // the average pool's backward does not look at its input: one launch over the stacked gradients
                    const Val& x = s0.x;
                    const long N = x.d[0], C = x.d[1], H = x.d[2], W = x.d[3];
                    Val gi = buf(m0, "gin.shared", {G * N, C, H, W}, NHWC);
                    emit([=](Run& c) { return k->avgpool2_backward(c.CS(), c.P(Gd), c.P(gi), (int)(G * N), (int)H, (int)W, (int)C); });
                    return share_gin(mods, gi);
                }
            }
            if (s0.shared_in) return gbwd_default(mods, ins, gouts, acc);
            return gbwd_stackable(mods, ins, gouts, acc);
        }
        case K_SDROP: {
            MS& s0 = S(m0);
            if (!(ran_stacked(m0) && m0.train)) return gbwd_stackable(mods, ins, gouts, acc);
            Val own = s0.noise; s0.noise = s0.noise_block;   // the stacked mask for the one stacked multiply
            vector<Val> r = gbwd_stackable(mods, ins, gouts, acc);
            S(m0).noise = own;
            return r;
        }
        case K_LINEAR: case K_CONV: {
            vector<Prep> gin;
            if (!prep_group(mods, gouts, &Compiler::prep_gin, "gin", false, gin)) return gbwd_default(mods, ins, gouts, acc);
            if (acc) wg_before_dgrad();
            emit_gemm(mods, gin, Epi(), false);
            vector<Val> outs;
            for (int b = 0; b < G; ++b) { S(*mods[b]).gin = gin[b].out; outs.push_back(gin[b].out); }
            if (acc) {
                wg_after_dgrad([&]() {
                    vector<PrepAcc> ap;
                    for (int b = 0; b < G; ++b) ap.push_back(prep_acc(*mods[b], gouts[b]));
                    emit_wgrad_group(mods, ap, S(m0).wg_ws, S(m0).wg_ws_bytes);
                });
            }
            return outs;
        }
        case K_PRELU: {
            if (!net->stacking) return gbwd_default(mods, ins, gouts, acc);
            const Val x0 = S(m0).x;
            vector<Val> xs; for (Mod* m : mods) xs.push_back(S(*m).x);
            Val X;
            const long n = x0.phys();
            if (net->fusion && stacked(xs, &X) && n % 4 == 0 && G <= 4) {
                // one launch for the G modules: stacked x / dy / dx, one slope and one gradient accumulator per group
                vector<Val> gs; for (auto& g : gouts) gs.push_back(match_fmt(g, x0));
                Val Gd = gather(m0, gs, x0);
                Val bs = x0; bs.d[0] *= G;
                Val dx = buf_like(m0, "gin.gblock", bs, x0.fmt);
                if (acc) ws_need(cg_prelu_backward_grouped_workspace_bytes(G, n));
                vector<Mod*> ms_ = mods;
                emit([=](Run& c) {
                    const float* al[4]; float* ga[4];
                    for (int b = 0; b < G; ++b) { al[b] = ms_[b]->w; ga[b] = ms_[b]->gw; }
                    return k->prelu_backward_grouped(c.CS(), c.P(X), c.P(Gd), al, c.P(dx), acc ? ga : nullptr, c.scale, G, n,
                                                     acc ? c.W() : nullptr, acc ? c.WB() : 0);
                });
                return share_gin(mods, dx);
            }
            seed_slices(mods, "gin", x0, x0.fmt);
            return gbwd_default(mods, ins, gouts, acc);
        }
        case K_SAMPLER: {
            MS& s0 = S(m0);
            bool plain = true; for (auto& g : gouts) plain = plain && g.fmt == PLAIN;
            if (s0.has_shared && !s0.out.none && s0.out.blk && s0.out.blk == s0.shared_out.key() && plain) {
                const Val img = ins[0].tab[0], grids = s0.shared_grids;
                const Val& gr0 = ins[0].tab[1];
                const long N = img.d[0], Hi = img.d[1], Wi = img.d[2], C = img.d[3], Ho = gr0.d[1], Wo = gr0.d[2];
                Val Gd = gather(m0, gouts, gouts[0]);
                Val gimg = buf(m0, "gimg.block", {G * N, Hi, Wi, C}), ggrid = buf(m0, "ggrid.block", {G * N, Ho, Wo, 2});
                emit([=](Run& c) { return k->bilinear_sampler_backward_shared(c.CS(), G, c.P(img), c.P(grids), c.P(Gd), c.P(gimg), c.P(ggrid), (int)N, (int)Hi, (int)Wi,
                                                                              (int)C, (int)Ho, (int)Wo); });
                vector<Val> gi = split(gimg, G), gg = split(ggrid, G), res;
                for (int b = 0; b < G; ++b) {
                    Val t; t.is_tab = true; t.none = false; t.tab = {gi[b], gg[b]};
                    S(*mods[b]).gin = t; res.push_back(t);
                }
                return res;
            }
            if (net->stacking) seed_slices(mods, "ggrid", ins[0].tab[1], PLAIN);
            return gbwd_default(mods, ins, gouts, acc);
        }
        default:
            if (stackable(m0)) return gbwd_stackable(mods, ins, gouts, acc);
            return gbwd_default(mods, ins, gouts, acc);
        }
    }

    // ---------------------------------------------------------------------------------------- backward of the fused segments
    vector<Val> bwd_act_pool(const vector<Mod*>& acts, const vector<Mod*>& pools, const vector<Mod*>& drops, const vector<Val>& gouts, bool acc) {
        const KTable* k = K();
        Mod &a0 = *acts[0], &p0 = *pools[0];
        MS& st = S(a0);
        const Val X = st.fX, mask = st.fmask; const int G = st.fG;
        const long N = st.fN, C = st.fC, H = st.fH, W = st.fW;
        vector<Val> gs; for (auto& g : gouts) gs.push_back(as_nhwc(g));
        Val Gd = gather(a0, gs, gs[0]);
        Val dx = buf_like(a0, "gin.fused", X, NHWC);
        const int code = a0.kind == K_PRELU ? 1 : 2;
        const float slope = code == 1 ? 0.f : a0.fa[0];
        const bool want = acc && code == 1;
        if (want) ws_need(cg_act_pool2_mask_backward_workspace_bytes(G, (int)N, (int)H, (int)W, (int)C));
        const int pool_max = p0.kind == K_MAXPOOL ? 1 : 0;
        const bool have_mask = !mask.none;
        vector<Mod*> ac = acts;
        emit([=](Run& c) {
            const float* al[4]; float* ga[4];
            for (int b = 0; b < G; ++b) { al[b] = ac[b]->w; ga[b] = ac[b]->gw; }
            return k->act_pool2_mask_backward(c.CS(), c.P(X), c.P(Gd), have_mask ? c.P(mask) : nullptr, c.P(dx), G, (int)N, (int)H, (int)W, (int)C, code, slope,
                                              code == 1 ? al : nullptr, want ? ga : nullptr, c.scale, pool_max, want ? c.W() : nullptr,
                                              want ? c.WB() : 0);
        });
        vector<Val> outs = slices(dx, G);
        for (int b = 0; b < G; ++b) {
            S(*acts[b]).gin = outs[b]; S(*pools[b]).gin = Val();
            if (!drops.empty()) S(*drops[b]).gin = Val();
        }
        return outs;
    }
    Val bwd_gemm_bn_act(Mod& conv, Mod& bn, Mod& act, const Val& in, const Val& go, bool acc) {
        const KTable* k = K();
        MS& sb = S(bn);
        const long Mr = sb.bnM, C = sb.bnC;
        const Val x = sb.x;
        Val dy = as_nhwc(go);
        Mod *bp = &bn, *ap = &act;
        Val sm = buf(bn, "save_mean", {C}), sv = buf(bn, "save_std", {C});
        Val b3 = buf(bn, "bsums3", {2 * C + 1}, PLAIN, 8);
        emit([=](Run& c) { return k->bn_act_backward_stats(c.CS(), c.P(x), c.P(dy), c.P(sm), c.P(sv), bp->w, bp->b, ap->w, Mr, (int)C, (double*)c.P(b3)); });
        Val gs = bn_sums_all(bn, b3, "bsums3_g", 2 * C + 1);
        Val dx = buf_like(bn, "gin", x, NHWC);
        const double cnt = sb.count;
        emit([=](Run& c) { return k->bn_act_backward(c.CS(), c.P(x), c.P(dy), bp->w, bp->b, c.P(sm), c.P(sv), ap->w, (const double*)c.P(gs), cnt, (const double*)c.P(b3),
                                                     Mr, (int)C, c.P(dx), acc ? bp->gw : nullptr, acc ? bp->gb : nullptr, acc ? ap->gw : nullptr, c.scale); });
        S(act).gin = Val(); sb.gin = dx;
        return bwd(conv, in, dx, acc);
    }

    // ---------------------------------------------------------------------------------------- data-parallel exchanges
    double dp_factor() const { return (net->world > 1 && net->sync_bn) ? (double)net->world : 1.0; }
    int bucket_done_upto = 0, bucket_ready = -1;
    enum { HOOK_ALLREDUCE_SUM = 0, HOOK_BUCKET_START = 1, HOOK_BUCKETS_FINISH = 2 };

    void emit_allreduce_sum(const Val& v, long count, int dtype) {   // sync-BN: in place SUM over ranks, ordered on the stream
        if (!(net->world > 1 && net->sync_bn)) return;
        emit([=](Run& c) -> int {
            Net* n = c.net;
            void* p = c.P(v);
            if (n->trace) { trace_note(n, "hook|allreduce_sum|" + TraceLine::pname(p) + "|" + std::to_string(count)); return 0; }
            if (n->comm_bn) {   // RCCL on the sync-BN communicator's stream, joined back into the compute stream (no host sync)
                if (cg_comm_allreduce(n->comm_bn, c.CS(), p, (size_t)count, dtype, 0)) return 1;
                if (cg_comm_wait(n->comm_bn, c.CS())) return 1;
                if (!(n->hook_too && n->hook)) return 0;
            }
            if (n->hook) return n->hook(n->hook_user, HOOK_ALLREDUCE_SUM, p, (size_t)count, dtype, c.CS()) ? cg::fail("cg_net: the host hook failed (sync-BN all-reduce of %ld elements)", count) : 0;
            return cg::fail("cg_net: world > 1 with sync-BN but neither a communicator (cg_net_set_dp) nor a host hook is set");
        });
        if (acc_pass && cs == 0) buckets_start();   // a bucket held back for this exchange (bucket_done) goes behind it
    }
    // Gradient buckets of the root nn.Sequential: each convolution / linear layer with the parameters of the modules
    // up to the next one is a contiguous range of the flat gradient vector; as soon as the backward walk has passed it, its all-reduce
    // starts on the gradient communicator's stream, under the backward of the layers in front of it.
    // Collectives of the two communicators are ordered on the device (comm.hip), and a bucket's all-reduce sits behind its layer's whole weight
    // gradient: started right away it would make the sync-BN exchange of the NEXT layer's backward - the first thing on the data-gradient
    // chain - wait for that weight gradient (157 us of stall per layer in the one-GPU dry run, profiles/r06_dp_dry_run.txt).  So while a
    // batch-norm layer in front still has its exchange to make, a complete bucket is held back and started right behind that exchange.
    void bucket_done(int first_module) {
        if (dry || !net->bucket_overlap || net->world <= 1) return;
        bucket_ready = first_module;
        bool bn_ahead = false;
        if (net->sync_bn) {
            const Mod& root = *net->mods[0];
            for (int t = 0; t < first_module && t < (int)root.kids.size(); ++t) {
                const Mod& m = *net->mods[root.kids[t]];
                bn_ahead = bn_ahead || (m.kind == K_BN && m.train);
            }
        }
        if (!bn_ahead) buckets_start();
    }
    void buckets_start() {
        if (dry || !net->bucket_overlap || net->world <= 1 || bucket_ready < 0 || bucket_ready >= bucket_done_upto) return;
        const int first_module = bucket_ready;
        for (int t = bucket_done_upto - 1; t >= first_module; --t) {
            for (size_t bi = 0; bi < pr->bucket_first.size(); ++bi) {
                if (pr->bucket_first[bi] != t) continue;
                // the bucket's weight gradients are on the weight-gradient stream (behind everything this stream has issued: fork here), maybe
                // still queued as deferred reductions; its collective starts from there
                wg_fork();
                const int s_ = wg_enter();
                flush_wgrad();
                // ... and on the weight-gradient streams of the branch groups behind it (D32_st3's nn.Concat: streams 5..7), which nothing
                // joins before the end of the pass: the collective's stream waits for what they hold so far (stream 0 does not)
                const int here = cs;
                for (int s = 0; s < 4; ++s) {
                    if (!wg_unjoined[s] || 4 + s == here) continue;
                    cs = 4 + s;
                    flush_wgrad();
                    emit_event(EV_RECORD, EV_WGJOIN, s);
                    cs = here;
                    emit_event(EV_WAIT, EV_WGJOIN, s);
                    wg_unjoined[s] = false;
                }
                wg_unjoined[s_] = false;
                float* ptr = pr->buckets[bi].first; const long cnt = pr->buckets[bi].second;
                emit([=](Run& c) -> int {
                    Net* n = c.net;
                    if (n->trace) { trace_note(n, "hook|bucket_start|" + TraceLine::pname(ptr) + "|" + std::to_string(cnt)); return 0; }
                    if (n->comm_grad) {
                        if (cg_comm_allreduce(n->comm_grad, c.CS(), ptr, (size_t)cnt, 0, 1)) return 1;
                        if (!(n->hook_too && n->hook)) return 0;
                        if (cg_comm_wait(n->comm_grad, c.CS())) return 1;   // the hook's transport reads what the collective wrote
                    }
                    if (n->hook) return n->hook(n->hook_user, HOOK_BUCKET_START, ptr, (size_t)cnt, 0, c.CS()) ? cg::fail("cg_net: the host hook failed (gradient bucket of %ld elements)", cnt) : 0;
                    return cg::fail("cg_net: bucketed all-reduce without a communicator or host hook");
                });
                wg_leave(s_);
            }
        }
        bucket_done_upto = first_module;
    }
};

}  // namespace
