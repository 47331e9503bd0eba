"""The validator V and its trainer on the MI355X against PyTorch-CPU restatements: nn.SoftMax, nn.BatchNormalization (1-D),
V's full forward / backward, one fevalV + Adam step, the device fake generator against its numpy twin, bit-reproducibility of a
seeded run, and train_v.py -> train.py --V_dir end to end."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import bulk_close, check_grads, close, snapshot, torch_twin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.mark.parametrize("rows,n", [(32, 2), (100, 2), (7, 1000), (5, 3000), (9, 37)])
def test_softmax_vs_torch(cg, rows, n):
    rs = np.random.RandomState(n)
    x = (rs.randn(rows, n) * 4).astype(np.float32)
    dy = rs.randn(rows, n).astype(np.float32)
    m = cg.nn.SoftMax()
    y = m.forward(cg.nn.to_device(x)).numpy()
    gi = m.backward(None, cg.nn.to_device(dy)).numpy()
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.softmax(xt, 1)
    yt.backward(torch.tensor(dy, dtype=torch.float64))
    close(y, yt.detach().numpy(), tol=2e-6, what="softmax y")
    close(gi, xt.grad.numpy(), tol=2e-6, what="softmax dx")


def _bn_setup(cg, N=32, n=1024):
    rs = np.random.RandomState(1)
    x = (rs.randn(N, n) * 3 + 1).astype(np.float32)
    dy = rs.randn(N, n).astype(np.float32)
    m = cg.nn.BatchNormalization(n)
    m.bias.copy(rs.randn(n).astype(np.float32) * 0.1)
    m.running_mean.copy(rs.randn(n).astype(np.float32) * 0.1)
    m.running_var.copy(rs.rand(n).astype(np.float32) + 0.5)
    return x, dy, m


def test_batchnorm_1d_training(cg):
    x, dy, m = _bn_setup(cg)
    w, b = m.weight.numpy(), m.bias.numpy()
    rm, rv = m.running_mean.numpy().astype(np.float64), m.running_var.numpy().astype(np.float64)
    y = m.forward(cg.nn.to_device(x)).numpy()
    gi = m.backward(None, cg.nn.to_device(dy)).numpy()
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    rmt, rvt = torch.tensor(rm), torch.tensor(rv)
    yt = F.batch_norm(xt, rmt, rvt, wt, bt, training=True, momentum=0.1, eps=1e-5)
    yt.backward(torch.tensor(dy, dtype=torch.float64))
    close(y, yt.detach().numpy(), tol=2e-5, what="bn1d y")
    close(gi, xt.grad.numpy(), tol=2e-5, what="bn1d dx")
    close(m.gradWeight.numpy(), wt.grad.numpy(), K=32, tol=2e-5, what="bn1d dgamma")
    close(m.gradBias.numpy(), bt.grad.numpy(), K=32, tol=2e-5, what="bn1d dbeta")
    close(m.running_mean.numpy(), rmt.numpy(), tol=2e-6, what="running mean")
    close(m.running_var.numpy(), rvt.numpy(), tol=2e-6, what="running var (unbiased)")


def test_batchnorm_1d_evaluate(cg):
    x, _, m = _bn_setup(cg)
    m.evaluate()
    y = m.forward(cg.nn.to_device(x)).numpy()
    yt = F.batch_norm(torch.tensor(x, dtype=torch.float64), torch.tensor(m.running_mean.numpy(), dtype=torch.float64),
                      torch.tensor(m.running_var.numpy(), dtype=torch.float64), torch.tensor(m.weight.numpy(), dtype=torch.float64),
                      torch.tensor(m.bias.numpy(), dtype=torch.float64), training=False, eps=1e-5)
    close(y, yt.numpy(), tol=2e-6, what="bn1d eval")


# ------------------------------------------------------------------------------ V against torch
def _fix_masks(V, N, rs, dims):
    """Explicit dropout masks (the fixed_noise test hook) for every dropout of V; returned by id(module) in the logical layout for torch."""
    masks = {}
    shape = None
    x_shapes = _shapes(V, N, dims)
    for i, m in enumerate(V.modules):
        shape = x_shapes[i]
        if m.typename == "nn.SpatialDropout":
            k = (rs.rand(N, shape[1]) >= m.p).astype(np.float32)
            m.fixed_noise = k
            masks[id(m)] = torch.tensor(k, dtype=torch.float64)[:, :, None, None]
        elif m.typename == "nn.Dropout":
            k = ((rs.rand(*shape) >= m.p) / (1 - m.p)).astype(np.float32)
            m.fixed_noise = k          # logical layout: a 4-D host array is stored NHWC like the map it masks
            masks[id(m)] = torch.tensor(k, dtype=torch.float64)
    return masks


def _shapes(V, N, dims):
    out = []
    shp = (N,) + tuple(dims)
    for m in V.modules:
        out.append(shp)
        t = m.typename
        if t == "nn.SpatialConvolution":
            shp = (N, m.nOutputPlane) + shp[2:]
        elif t == "nn.SpatialMaxPooling":
            shp = (N, shp[1], shp[2] // 2, shp[3] // 2)
        elif t == "nn.View":
            shp = (N, m.sizes[0])
        elif t == "nn.Linear":
            shp = (N, m.weight.shape[0])
    return out


def _bce(p, t):
    eps = 1e-12
    return -(t * torch.log(p + eps) + (1 - t) * torch.log(1 - p + eps)).mean()


@pytest.mark.parametrize("dims,N", [((3, 32, 32), 32), ((1, 32, 32), 32), ((3, 64, 64), 8), ((3, 16, 16), 16)])
def test_v_forward_backward_vs_torch(cg, dims, N):
    cg.manual_seed(11)
    V = cg.models.create_V(dims)
    _, G = V.getParameters()
    rs = np.random.RandomState(3)
    x = rs.rand(N, *dims).astype(np.float32)
    t = np.zeros((N, 2), np.float32)
    t[: N // 2, 1] = 1
    t[N // 2:, 0] = 1
    masks = _fix_masks(V, N, rs, dims)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    params, taps = [], {}
    yt = torch_twin(V, snapshot(V), xt, params, taps, masks=masks)
    loss = _bce(yt, torch.tensor(t, dtype=torch.float64))
    loss.backward()
    crit = cg.nn.BCECriterion()
    G.zero()
    y = V.forward(cg.nn.to_device(x))
    f = crit.forward(y, cg.nn.to_device(t))
    gi = V.backward(cg.nn.to_device(x), crit.backward(y, cg.nn.to_device(t)))
    close(cg.nn.as_plain(y).numpy(), yt.detach().numpy(), tol=1e-4, what="V output")
    close(float(f), float(loss.detach()), tol=1e-4, what="loss")
    bulk_close(cg.nn.as_plain(gi).numpy(), xt.grad.numpy(), what="V gradInput")
    check_grads(G.numpy(), params)
    for m in V.modules:
        if "BatchNormalization" in m.typename:
            rm, rv = taps[id(m)]
            close(m.running_mean.numpy(), rm.numpy(), tol=1e-4, what="running mean")
            close(m.running_var.numpy(), rv.numpy(), tol=1e-4, what="running var")


def _bank():
    syn = importlib.import_module("cat-generator_amd.synthetic")
    return syn.create_overlay_bank(32, 32, np.random.RandomState(5), n=64, n_points=3000)


def test_fevalV_adam_step_vs_torch(cg):
    tv = importlib.import_module("train_v")
    cg.manual_seed(2)
    T = tv.VTrainer(cg, (3, 32, 32), dict(seed=2, batchSize=32, V_L1=0.0, V_L2=0.01, V_clamp=5.0, N_epoch=32), bank=_bank())
    pool = cg.adversarial.TrainData(np.random.RandomState(9).rand(40, 3, 32, 32).astype(np.float32))
    N = 32
    rs = np.random.RandomState(4)
    masks = _fix_masks(T.V, N, rs, (3, 32, 32))
    p0 = T.PARAMETERS_V.numpy().copy()
    snap = snapshot(T.V)                                       # the values before the step, for the torch restatement
    b = T.batch(pool, N)
    x = cg.nn.as_plain(b["inputs"]).numpy()
    t = b["targets"].numpy()
    # teacher-forced: the batch above, then fevalV + adam exactly as step() runs them
    import types
    T.batch = types.MethodType(lambda self, *a, **k: b, T)
    last = T.step(pool, N)
    torch.cuda.synchronize()
    xt = torch.tensor(x, dtype=torch.float64)
    params = []
    yt = torch_twin(T.V, snap, xt, params, {}, masks=masks)
    loss = _bce(yt, torch.tensor(t, dtype=torch.float64))
    loss.backward()
    gref = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    close(float(last["f"]), float(loss.detach()), tol=1e-4, what="loss")
    g = T.GRAD_PARAMETERS_V.numpy().astype(np.float64)          # what fevalV handed to adam: penalty + clamp applied
    bulk_close(g, np.clip(gref + 0.01 * p0, -5, 5), what="clamped gradient")
    st = T.OPTSTATE["adam"]
    m, v = st["m"].numpy().astype(np.float64), st["v"].numpy().astype(np.float64)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=1e-4, atol=1e-20)     # (1 - beta2) g^2 rounded in fp32
    step = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (np.sqrt(v) + 1e-8)   # Torch7 adam: eps outside the bias correction
    np.testing.assert_allclose(T.PARAMETERS_V.numpy(), p0 - step, rtol=0, atol=2e-7)


# ------------------------------------------------------------------------------ the device generator
@pytest.mark.parametrize("dims", [(3, 32, 32), (1, 32, 32)])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("second", [False, True])
def test_generator_matches_numpy_twin(cg, dims, kind, second):
    syn = cg.synthetic
    rs = np.random.RandomState(kind * 2 + int(second))
    gen = syn.Generator(dims, rs, bank=_bank())
    pool_np = np.random.RandomState(1).rand(24, *dims).astype(np.float32)
    pool = cg.adversarial.TrainData(pool_np).pool
    plan = gen.draw(16, 24, kind=kind, second=second)
    out = cg.Tensor.empty((16,) + dims, "nhwc")
    gen.run(plan, pool, out.ptr)
    dev = out.numpy()
    K, (C, H, W) = plan.n_overlays, dims
    dev_ov = gen._dev["ovl"][:K * H * W].cpu().numpy().reshape(K, H, W)
    ov = syn.plan_overlays_np(gen, plan)
    assert np.abs(dev_ov - ov).max() <= 1e-6, "overlay composition (cg_synth_overlays) against the twin"
    # the images from the same overlays: the Warp kind moves pixels by (2o - 1) * length, which scales an overlay's last-bit
    # difference by up to 10 before the bilinear read, so each stage is held to the bound on its own inputs
    ref = syn.synth_images_np(pool_np, dev_ov, plan.idesc, plan.fdesc)
    err = np.abs(dev - ref).max(axis=(1, 2, 3))
    assert np.all(err <= 1e-6 * ref.max(axis=(1, 2, 3))), f"max |device - twin| per image: {err}"
    assert np.all(dev.max(axis=(1, 2, 3)) == 1.0) and dev.min() >= 0


def test_seeded_v_training_is_bit_reproducible(cg):
    tv = importlib.import_module("train_v")
    bank = _bank()
    pool = cg.adversarial.TrainData(np.random.RandomState(3).rand(48, 3, 32, 32).astype(np.float32))
    runs = []
    for _ in range(2):
        cg.manual_seed(7)
        T = tv.VTrainer(cg, (3, 32, 32), dict(seed=7, batchSize=32, N_epoch=96), bank=bank)
        for _ in range(3):
            T.step(pool, 32)
        torch.cuda.synchronize()
        runs.append((T.PARAMETERS_V.numpy().copy(), T.CONFUSION.counts.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][1].sum() == 96


def _run(args, timeout=420):
    env = dict(os.environ)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + args, cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, f"{args[0]} exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def test_train_v_then_train_rates_with_v(tmp_path):
    vdir, gdir, gdir2 = tmp_path / "v", tmp_path / "g", tmp_path / "g2"
    out = _run(["train_v.py", "--synthetic", "--N_epoch", "64", "--batchSize", "32", "--epochs", "2", "--saveFreq", "1",
                "--save", str(vdir)])
    assert (vdir / "v_3x32x32.net").exists() and "time to learn 1 sample" in out
    assert any(p.suffix == ".png" for p in (vdir / "v_rated_real").glob("*")) or any((vdir / "v_rated_fake").glob("*.png"))
    out = _run(["train.py", "--synthetic", "--epochs", "1", "--N_epoch", "64", "--V_dir", str(vdir), "--save", str(gdir)])
    assert "[V] semiRandom" in out and "goodImages" in out and "badImages" in out
    out = _run(["train.py", "--synthetic", "--epochs", "1", "--N_epoch", "64", "--V_dir", str(tmp_path / "none"), "--save", str(gdir2)])
    assert "[V] semiRandom" not in out and "no validator network" in out
