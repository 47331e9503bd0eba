"""--D_diffaug on the device: the differentiable augmentation T of D's input and its adjoint (csrc/diffaug.hip, cg_diffaug_forward /
cg_diffaug_backward), then the trainer with the flag.

Kernels, through the C ABI over their dispatch edges - the float4 form, the scalar twin behind a pointer 4 bytes off a 16-byte boundary
or a C H W that 4 does not divide, one image and more images than a wave of workgroups, the 48 KB stage and the 64 KB one - with two
measures:
  bits_equal      the stored descriptors against the host twin diffaug.draw_np; draw = 1 against draw = 0 on those descriptors; in place
                  against out of place; a second call; an image at another index of another batch; policies without colour (pure moves
                  and zeros) against the restatement
  rounding_close  policies with colour against the fp64 restatement diffaug.forward_np / backward_np on the device's descriptors, terms
                  from diffaug_ref (the magnitudes of the addends of (v - m) k + m), r counted below from the formulas include/catgan.h
                  fixes: fmaf(v - m, k, m), the channel mean ((v0 + v1) + v2) / 3, the image mean one rounding of an fp64 sum
Roundings on the longest chain, forward, C = 3 (csrc/diffaug.hip diffaug_fwd_k, its pixel and output loops):
  x1 = x + b                      1
  m  = ((x1 + x1') + x1'') / 3    + 3 = 4      (saturate)
  x2 = fmaf(x1 - m, s, m)         + 2 = 6      (mix)
  M  = (float)(fp64 sum / L)      + 1 = 7      (block_mean)
  x3 = fmaf(x2 - M, c, M)         + 2 = 9      (mix)                  r = 9 + 2 = 11;  C = 1 has no saturation: 1 + 1 + 2 = 4, r = 6
backward, C = 3 (diffaug_bwd_k's output loop): Gm 1, g3 = fmaf(g2 - Gm, c, Gm) + 2 = 3, m + 3 = 6, dx = fmaf(g3 - m, s, m) + 2 = 8,
r = 10;  C = 1: 1 + 2 = 3, r = 5."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffaug_ref as R
from helpers import bits_equal, dev, edge_normal, host, out_like, rounding_close

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_FWD = {3: 11, 1: 6}          # the docstring's count: x3's chain through m and M, + 2
R_BWD = {3: 10, 1: 5}          # dx's chain through Gm and m, + 2
SEED, OFF = 11, 1000003
COLOR = 1


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def da(cg):
    return importlib.import_module("cat-generator_amd.diffaug")


def fwd(cg, x, y, desc, shape, policy, draw, offset=OFF, base=None):
    N, H, W, C = shape
    cg.lib().diffaug_forward(cg.tensor.stream(), x.data_ptr(), y.data_ptr(), desc.data_ptr(), N, H, W, C, policy, draw, SEED, offset, base)


def bwd(cg, gy, gx, desc, shape, policy):
    N, H, W, C = shape
    cg.lib().diffaug_backward(cg.tensor.stream(), gy.data_ptr(), gx.data_ptr(), desc.data_ptr(), N, H, W, C, policy)


def n_of(shape):
    return int(np.prod(shape))


# ------------------------------------------------------------------------------ 1. the kernels over their dispatch edges
# N, H, W, C.  6 x 10 x 3 = 180 floats (4 divides it: float4, and its scalar twin off alignment), non-square; 5 x 7 x 3 = 105: the scalar
# twin at any alignment; 130 images: more workgroups than half the CUs; 64 x 64 x 3: 48 KB of LDS; 128 x 128 x 1: the 64 KB limit itself
SHAPES = [(1, 6, 10, 3), (3, 6, 10, 3), (3, 5, 7, 3), (5, 16, 16, 1), (130, 32, 32, 3), (2, 64, 64, 3), (1, 128, 128, 1)]


@functools.lru_cache(maxsize=None)
def data(shape):
    """x, g and the descriptors draw_np gives at (SEED, OFF): computed once per shape, never written to"""
    da = R.da()
    rng = np.random.default_rng(n_of(shape))
    x, g = edge_normal(rng, shape), edge_normal(rng, shape)
    desc = da.draw_np(SEED, OFF, shape[0], shape[1], shape[2])
    return x, g, desc


@functools.lru_cache(maxsize=None)
def reference(shape, policy):
    da = R.da()
    x, g, desc = data(shape)
    return (da.forward_np(x, desc, policy), R.forward_terms(x, desc, policy), da.backward_np(g, desc, policy), R.backward_terms(g, desc, policy))


def check_against_restatement(got, ref, terms, policy, r, what):
    if policy & COLOR:
        rounding_close(got, ref.reshape(-1), terms.reshape(-1), r, what)
    else:
        bits_equal(got, ref.astype(f32).reshape(-1), what)          # moves and zeros: the restatement's values are fp32 values


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "off16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_over_the_dispatch_edges(cg, da, shape, mis):
    N, H, W, C = shape
    x, g, desc_np = data(shape)
    n = n_of(shape)
    for policy in range(1, 8):
        what = f"{shape}, policy {policy}, {'4 bytes off' if mis else 'aligned'}"
        yref, yterms, gref, gterms = reference(shape, policy)
        # ---- forward: draw = 1 stores draw_np's descriptors; draw = 0 on them gives the same image
        xd, y1, d1 = dev(x, mis), out_like(n, mis), dev(np.full((N, 8), 9.0, f32))
        fwd(cg, xd, y1, d1, shape, policy, 1)
        bits_equal(host(d1, (N, 8)), desc_np, f"stored descriptors vs draw_np, {what}")
        y1h = host(y1)
        bits_equal(host(xd), x.reshape(-1), f"x left alone, {what}")
        y0 = out_like(n, mis)
        dd = dev(desc_np)
        fwd(cg, xd, y0, dd, shape, policy, 0)
        bits_equal(host(y0), y1h, f"draw = 0 vs draw = 1, {what}")
        bits_equal(host(dd, (N, 8)), desc_np, f"draw = 0 left the descriptors alone, {what}")
        fwd(cg, xd, y0, dd, shape, policy, 0)
        bits_equal(host(y0), y1h, f"a second call, {what}")
        xin = dev(x, mis)
        fwd(cg, xin, xin, d1, shape, policy, 1)
        bits_equal(host(xin), y1h, f"in place vs out of place, {what}")
        check_against_restatement(y1h, yref, yterms, policy, R_FWD[C], f"forward vs fp64, {what}")
        # ---- backward, on the same descriptors
        gd, gx = dev(g, mis), out_like(n, mis)
        bwd(cg, gd, gx, dd, shape, policy)
        gxh = host(gx)
        bits_equal(host(gd), g.reshape(-1), f"gy left alone, {what}")
        bwd(cg, gd, gx, dd, shape, policy)
        bits_equal(host(gx), gxh, f"backward, a second call, {what}")
        bwd(cg, gd, gd, dd, shape, policy)
        bits_equal(host(gd), gxh, f"backward in place vs out of place, {what}")
        check_against_restatement(gxh, gref, gterms, policy, R_BWD[C], f"backward vs fp64, {what}")
        # ---- an image's result depends neither on N nor on its position: the batch reversed, and its last image alone
        rev = np.ascontiguousarray(x[::-1]), np.ascontiguousarray(g[::-1]), dev(np.ascontiguousarray(desc_np[::-1]))
        y2, g2 = out_like(n, mis), out_like(n, mis)
        fwd(cg, dev(rev[0], mis), y2, rev[2], shape, policy, 0)
        bwd(cg, dev(rev[1], mis), g2, rev[2], shape, policy)
        per = n // N
        bits_equal(host(y2, (N, per))[::-1].reshape(-1), y1h, f"forward, the batch reversed, {what}")
        bits_equal(host(g2, (N, per))[::-1].reshape(-1), gxh, f"backward, the batch reversed, {what}")
        one = (1,) + shape[1:]
        y3, g3, d3 = out_like(per, mis), out_like(per, mis), dev(desc_np[N - 1:])
        fwd(cg, dev(x[N - 1:], mis), y3, d3, one, policy, 0)
        bwd(cg, dev(g[N - 1:], mis), g3, d3, one, policy)
        bits_equal(host(y3), y1h[(N - 1) * per:], f"forward, the last image alone, {what}")
        bits_equal(host(g3), gxh[(N - 1) * per:], f"backward, the last image alone, {what}")


def test_the_device_base_moves_the_draws(cg, da):
    """offset + *base + 8 n + k (cg_rng_*_dev semantics): what a captured iteration replays with"""
    shape = (3, 6, 10, 3)
    x, _, _ = data(shape)
    base = torch.tensor([4242], dtype=torch.int64, device="cuda")
    d = dev(np.zeros((3, 8), f32))
    fwd(cg, dev(x), out_like(n_of(shape)), d, shape, 7, 1, base=base.data_ptr())
    bits_equal(host(d, (3, 8)), da.draw_np(SEED, OFF + 4242, 3, 6, 10), "descriptors drawn behind the device base")
    assert int(base.item()) == 4242


@pytest.mark.parametrize("shape", [(6, 10, 3), (5, 7, 3), (16, 16, 1)], ids=lambda s: "x".join(map(str, s)))
def test_hand_placed_descriptors(cg, da, shape):
    """Every combination of the extreme draws - tx = +-Rw, ty = +-Rh, cy in {0, H}, cx in {0, W}, s in {0, 1}, c in {0.5, 1}, b = 0 - one
    image each, and two images moved out of the picture altogether (tx = W, ty = -H), through draw = 0."""
    H, W, C = shape
    Rh, Rw, _, _ = R.half_sizes(H, W)
    rows = [(0.0, s, c, tx, ty, cy, cx, 0.0) for tx in (-Rw, Rw) for ty in (-Rh, Rh) for cy in (0, H) for cx in (0, W) for s in (0.0, 1.0)
            for c in (0.5, 1.0)]
    rows += [(0.0, 1.0, 1.0, W, 0, 0, 0, 0.0), (0.0, 0.5, 0.75, 0, -H, H, W, 0.0)]
    desc = np.array(rows, f32)
    N = len(rows)
    full = (N, H, W, C)
    rng = np.random.default_rng(H * W)
    x, g = edge_normal(rng, full), edge_normal(rng, full)
    for policy in range(1, 8):
        what = f"{shape}, policy {policy}, hand-placed"
        dd, y, gx = dev(desc), out_like(n_of(full)), out_like(n_of(full))
        fwd(cg, dev(x), y, dd, full, policy, 0)
        bwd(cg, dev(g), gx, dd, full, policy)
        yh, gh = host(y, full), host(gx, full)
        check_against_restatement(yh.reshape(-1), da.forward_np(x, desc, policy), R.forward_terms(x, desc, policy), policy, R_FWD[C], "forward, " + what)
        check_against_restatement(gh.reshape(-1), da.backward_np(g, desc, policy), R.backward_terms(g, desc, policy), policy, R_BWD[C], "backward, " + what)
        if policy & 2:       # moved out of the picture: nothing of x arrives, and nothing of g comes back but the contrast's mean (zero)
            assert not yh[N - 2:].any() and not gh[N - 2:].any()


# ------------------------------------------------------------------------------ 2. the trainer
PX, BATCH, POLICY = 16, 8, "color,translation,cutout"


def make_state(cg, seed, **opt):
    cg.manual_seed(seed)
    dims = (3, PX, PX)
    G, D = cg.models.create_G(dims, 100), cg.models.create_D(dims)
    return cg.adversarial.State(dict(batchSize=BATCH, scale=PX, seed=4, **opt), G, D)


def make_data(cg):
    return cg.adversarial.TrainData(np.random.RandomState(10).rand(32, 3, PX, PX).astype(f32))


def opt_tensors(cg, S):
    out = {}
    for method, per_net in S.OPTSTATE.items():
        for net, stt in per_net.items():
            for k, v in stt.items():
                if isinstance(v, cg.tensor.Tensor):
                    out[f"{method}/{net}/{k}"] = v.numpy()
    return out


def nhwc(t):
    """an engine tensor ([N,C,H,W] logical) as the kernels see it"""
    return np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))


def run(cg, iters=3, keep=False, **opt):
    """iters eager iterations; -> the state, per-iteration S._last (with keep: 4-D tensors as [N][H][W][C] arrays), the counter position
    after each, the last iteration's trace"""
    S = make_state(cg, 21, **opt)
    S.keep_outputs = keep
    dset = make_data(cg)
    lasts, offs = [], [cg.tensor.rng().offset]
    for k in range(iters):
        cg.lib().trace = [] if k == iters - 1 else None
        cg.adversarial.iteration(S, dset, BATCH)
        calls, cg.lib().trace = cg.lib().trace, None
        if keep:     # host copies now: the buffers behind S._last["samples"] are reused by the next iteration
            lasts.append({k: (nhwc(v) if isinstance(v, cg.tensor.Tensor) and v.dim() == 4 else v) for k, v in dict(S._last, fake=S._last_fake).items()})
        offs.append(cg.tensor.rng().offset)
    torch.cuda.synchronize()
    return S, lasts, offs, calls


def same_state(cg, A, B, what):
    bits_equal(A.PARAMETERS_G.numpy(), B.PARAMETERS_G.numpy(), "PARAMETERS_G, " + what)
    bits_equal(A.PARAMETERS_D.numpy(), B.PARAMETERS_D.numpy(), "PARAMETERS_D, " + what)
    ta, tb = opt_tensors(cg, A), opt_tensors(cg, B)
    assert ta.keys() == tb.keys() and {"adam/D/m", "adam/D/v", "adam/G/m", "adam/G/v"} <= ta.keys()
    for k in ta:
        bits_equal(ta[k], tb[k], f"optimiser state {k}, {what}")


def test_flag_off_is_the_run_it_always_was(cg):
    """A State whose OPT never held the key, and one whose key says off: the same entry points with the same scalar arguments, the same
    parameters, optimiser state and counter position, and no cg_diffaug_* call."""
    A, _, offA, callsA = run(cg)
    B, _, offB, callsB = run(cg, D_diffaug="none")
    assert A.DIFFAUG is None and B.DIFFAUG is None and "D_diffaug" not in A.OPT
    names = [c for c, _ in callsA]
    assert names == [c for c, _ in callsB] and not [c for c in names if "diffaug" in c]
    assert offA == offB
    same_state(cg, A, B, "flag off vs no flag")


def d_calls(S, calls):
    """the trace reduced to T's calls and D's passes"""
    hd = S.MODEL_D._pnet[1].h.value
    return [(c, a) for c, a in calls if "diffaug" in c or (c in ("cg_net_forward", "cg_net_backward") and getattr(a[0], "value", a[0]) == hd)]


def test_flag_on_trace_and_counter_stream(cg):
    on, _, off_on, calls_on = run(cg, D_diffaug=POLICY)
    off, _, off_off, calls_off = run(cg)
    seq = d_calls(on, calls_on)
    assert [c for c, _ in seq] == ["cg_diffaug_forward", "cg_net_forward", "cg_net_backward",
                                   "cg_diffaug_forward", "cg_net_forward", "cg_net_backward", "cg_diffaug_backward"], [c for c, _ in seq]
    # D's first pass reads the batch T wrote in place; its second one the buffer T wrote the samples into; the adjoint uses the G-step's draws
    (_, f1), (_, n1), _, (_, f2), (_, n2), _, (_, b1) = seq
    assert f1[1] == f1[2] == n1[2] and f2[1] != f2[2] and f2[2] == n2[2]
    assert f1[3] != f2[3] and b1[3] == f2[3]
    assert f1[8] == f2[8] == b1[8] == 7 and f1[9] == f2[9] == 1
    # nothing else in the iteration changes
    assert [c for c, _ in calls_on if "diffaug" not in c] == [c for c, _ in calls_off]
    # two forwards of 8 counters per image per iteration, whatever the policy
    assert [a - b for a, b in zip(off_on, off_off)] == [k * 2 * 8 * BATCH for k in range(4)]
    one, _, off_one, _ = run(cg, D_diffaug="cutout")
    assert off_one == off_on
    # D_iterations = 2: a fresh draw for each D iteration
    two, _, off_two, calls_two = run(cg, iters=1, D_diffaug=POLICY, D_iterations=2)
    _, _, off_two_off, _ = run(cg, iters=1, D_iterations=2)
    t = [(c, a) for c, a in calls_two if "diffaug" in c]
    assert [c for c, _ in t] == ["cg_diffaug_forward"] * 3 + ["cg_diffaug_backward"]
    assert len({a[11] for _, a in t[:3]}) == 3, "the three forwards drew from the same counters"
    assert off_two[1] - off_two_off[1] == 3 * 8 * BATCH


def test_flag_on_what_D_saw_and_what_G_got(cg, da):
    S, lasts, offs, _ = run(cg, keep=True, D_diffaug=POLICY)
    seed = cg.tensor.rng().seed
    descs = []
    for k, last in enumerate(lasts):
        dD, dG = last["desc_D"], last["desc_G"]
        descs += [dD, dG]
        # D's batch: real rows and G's fakes, both halves through T
        inputs = last["inputs_D"]
        bits_equal(inputs[BATCH // 2:], last["fake"], f"iteration {k}: the fake half of D's batch is G's un-augmented output")
        rounding_close(last["aug_D"], da.forward_np(inputs, dD, 7), R.forward_terms(inputs, dD, 7), R_FWD[3], f"iteration {k}: the batch D saw")
        # the G-step: samples stay as G made them, D sees T(samples), G gets T^T of D's input gradient
        samples = last["samples"]
        rounding_close(last["aug_G"], da.forward_np(samples, dG, 7), R.forward_terms(samples, dG, 7), R_FWD[3], f"iteration {k}: the samples D saw")
        assert not np.array_equal(last["aug_G"], samples)
        gD = last["gradInput_D"]
        assert np.abs(gD).max() > 0
        rounding_close(last["df_G"], da.backward_np(gD, dG, 7), R.backward_terms(gD, dG, 7), R_BWD[3], f"iteration {k}: the gradient handed to G")
    # the draws: the first D-step's lie right behind its fake images' noise (4 rows of 100) in the counter stream
    bits_equal(descs[0], da.draw_np(seed, offs[0] + (BATCH // 2) * 100, BATCH, PX, PX), "the first D-step's descriptors")
    # fresh in either step of an iteration and in every iteration
    for i in range(len(descs)):
        for j in range(i + 1, len(descs)):
            assert not np.array_equal(descs[i][:, :7], descs[j][:, :7]), f"draws {i} and {j} are the same"


def test_flag_on_both_orders_of_the_generator_forwards_agree(cg):
    """CG_CONCURRENT_G_BOTH = 0 and = 1 (OPT.concurrent_g_both): T's draws sit at the same counters in either order of calls"""
    A, _, offA, _ = run(cg, D_diffaug=POLICY, concurrent_g_both=True)
    B, _, offB, _ = run(cg, D_diffaug=POLICY, concurrent_g_both=False)
    assert offA == offB
    same_state(cg, A, B, "concurrent_g_both on vs off")
    C, _, _, _ = run(cg)
    assert not np.array_equal(A.PARAMETERS_D.numpy(), C.PARAMETERS_D.numpy()), "the flag changed nothing"


def test_flag_on_graph_replay_matches_eager(cg):
    """2 eager + 1 replayed iteration through GraphedIteration against 3 eager ones with the same device-side counters"""
    def go(graph):
        S = make_state(cg, 41, D_diffaug=POLICY)
        dset = make_data(cg)
        r = cg.tensor.rng()
        if graph:
            it = cg.adversarial.GraphedIteration(S, dset, BATCH, warmup=2)
            it()
        else:
            S.device_rng = True
            for k in ("D", "G"):
                S.OPTSTATE["adam"][k]["device_step"] = True
            r.enable_device_base()
            for _ in range(3):
                off0 = r.offset
                cg.adversarial.iteration(S, dset, BATCH)
                cg.lib().counter_add(cg.tensor.stream(), r.dev_base.data_ptr(), r.offset - off0)
                r.offset = off0
        torch.cuda.synchronize()
        return S, r.offset + int(r.dev_base.item()), S.DIFFAUG.desc_np("D", BATCH), S.DIFFAUG.desc_np("G", BATCH)
    G, offG, dDg, dGg = go(True)
    E, offE, dDe, dGe = go(False)
    assert offG == offE
    bits_equal(dDg, dDe, "the last D-step's descriptors, replay vs eager")
    bits_equal(dGg, dGe, "the last G-step's descriptors, replay vs eager")
    same_state(cg, G, E, "replay vs eager")


def test_flag_on_resume_is_bit_for_bit(cg, tmp_path):
    dset = make_data(cg)
    A = make_state(cg, 72, D_diffaug=POLICY)
    for _ in range(2):
        cg.adversarial.iteration(A, dset, BATCH)
    ck = cg.checkpoint.save(str(tmp_path / "a.npz"), A)
    for _ in range(2):
        cg.adversarial.iteration(A, dset, BATCH)
    offA = cg.tensor.rng().offset
    B = make_state(cg, 72, D_diffaug=POLICY)
    cg.checkpoint.load(ck, B)
    assert B.OPT["D_diffaug"] == POLICY
    for _ in range(2):
        cg.adversarial.iteration(B, dset, BATCH)
    torch.cuda.synchronize()
    assert cg.tensor.rng().offset == offA
    same_state(cg, A, B, "after the resume")
    bits_equal(B.DIFFAUG.desc_np("G", BATCH), A.DIFFAUG.desc_np("G", BATCH), "the last descriptors after the resume")


def test_train_py_runs_with_the_flag(cg, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--epochs", "1", "--N_epoch", "64", "--batchSize", "8", "--scale", "16",
           "--D_diffaug", POLICY, "--save", str(tmp_path / "logs"), "--V_dir", str(tmp_path / "nov"), "--G_pretrained_dir", str(tmp_path / "nog")]
    r = subprocess.run(["timeout", "-k", "10", "240"] + cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "trained D" in r.stdout
