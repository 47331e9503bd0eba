"""Generator pre-training on the MI355X: cg_mse_forward / cg_mse_backward against nn_utils.mse_np (every length either side of the
kernel's tile, chunk and partial-count boundaries, both alignment paths), nn.MSECriterion across storage formats, the auto-encoder's
forward / backward and one fevalG + Adam step against a torch fp64 CPU twin, bit-reproducibility of a seeded pretrain_g.py run, and
pretrain_g.py -> train.py --G_pretrained_dir end to end."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import KINK, bulk_close, check_grads, close, snapshot, torch_twin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


# ------------------------------------------------------------------------------ the kernels against mse_np
CHUNK, PARTS = 4096, 1024             # nn_utils.MSE_CHUNK / MSE_MAX_PARTIALS: asserted below
QUADS = 1024                          # one pass of a workgroup: 256 threads x 4 elements
LENGTHS = [1, 3, 63, 64, 65, 255, 256, 257,                        # a wave of scalar lanes, a wave of quads (256 elements)
           QUADS - 1, QUADS, QUADS + 1,                            # one pass of the 256 threads
           CHUNK - 4, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4,      # one workgroup / two partials (the smallest multi-partial length)
           2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 49152, 49154,
           255 * CHUNK + 8, 256 * CHUNK, 256 * CHUNK + 3, 257 * CHUNK,   # partials: one each for the finishing threads, then two for the first
           CHUNK * PARTS - 4, CHUNK * PARTS, CHUNK * PARTS + 1, CHUNK * PARTS + 4]   # beyond: workgroups walk a second chunk (grid-stride)


def _ulp_close(a, ref, what):
    a, ref = np.float32(a), np.float32(ref)
    assert abs(np.float64(a) - np.float64(ref)) <= np.spacing(np.abs(ref)), f"{what}: {a!r} vs {ref!r}"


def _dev(a, offset):
    """a on the device, `offset` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + a.size]
    v.copy_(torch.from_numpy(a))
    return v


def _run_mse(cg, x, t, offset=0):
    L, s = cg.lib(), cg.tensor.stream()
    dx_, dt_ = _dev(x, offset), _dev(t, offset)
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    g = torch.full((x.size + 8,), np.nan, dtype=torch.float32, device="cuda")
    gv = g[offset:offset + x.size]
    L.mse_forward(s, dx_.data_ptr(), dt_.data_ptr(), loss.data_ptr(), x.size)
    L.mse_backward(s, dx_.data_ptr(), dt_.data_ptr(), gv.data_ptr(), x.size)
    torch.cuda.synchronize()
    out = g.cpu().numpy()
    assert np.isnan(out[:offset]).all() and np.isnan(out[offset + x.size:]).all(), "cg_mse_backward wrote outside dx"
    return loss.cpu().numpy()[0], out[offset:offset + x.size]


_DATA = {}


def _data(cg, n):
    """(x, t, mse_np's loss and gradient) for a length: computed once, shared by the tests, never written."""
    if n not in _DATA:
        rs = np.random.RandomState(n % 100003)
        x, t = rs.randn(n).astype(np.float32), rs.rand(n).astype(np.float32)
        loss, g = cg.nn_utils.mse_np(x, t)
        for a in (x, t, g):
            a.setflags(write=False)
        _DATA[n] = (x, t, loss, g)
    return _DATA[n]


@pytest.mark.parametrize("n", LENGTHS)
def test_mse_kernel_vs_numpy(cg, n):
    assert (cg.nn_utils.MSE_CHUNK, cg.nn_utils.MSE_MAX_PARTIALS) == (CHUNK, PARTS)
    x, t, ref_loss, ref_g = _data(cg, n)
    loss, g = _run_mse(cg, x, t)                        # 16-byte path when n % 4 == 0, scalar otherwise
    print(f"n={n}: loss {loss!r} mse_np {ref_loss!r}")
    assert np.array_equal(g, ref_g), "gradient is not bit-equal to mse_np"
    _ulp_close(loss, ref_loss, "loss")
    loss2, g2 = _run_mse(cg, x, t)
    assert loss.tobytes() == loss2.tobytes() and np.array_equal(g, g2), "two runs differ"
    # pointers one float past the boundary: the scalar path, on the same data -> the same bits
    loss3, g3 = _run_mse(cg, x, t, offset=1)
    assert np.array_equal(g3, ref_g)
    assert loss3.tobytes() == loss.tobytes(), f"aligned {loss!r} and misaligned {loss3!r} paths differ"


def test_mse_planted_cases(cg):
    for n in (4096, 4097, 49152):
        x = np.random.RandomState(n).randn(n).astype(np.float32)
        loss, g = _run_mse(cg, x, x.copy())
        assert loss == 0.0 and not g.any()
    for pos in (0, 2048, 4096):           # one differing element among 4096 zeros, in the first chunk and alone in the second
        x, t = np.zeros(4097, np.float32), np.zeros(4097, np.float32)
        x[pos] = 1e-3
        ref_loss, ref_g = cg.nn_utils.mse_np(x, t)
        loss, g = _run_mse(cg, x, t)
        assert loss > 0 and ref_loss > 0
        _ulp_close(loss, ref_loss, f"planted at {pos}")
        assert np.array_equal(g, ref_g) and g[pos] != 0 and np.count_nonzero(g) == 1
    # what fp32 accumulation would lose: 4096 squares of 1e-6 beside one of 1e8
    x = np.full(4097, 1e-3, np.float32)
    x[0] = 1e4
    t = np.zeros_like(x)
    loss, _ = _run_mse(cg, x, t)
    _ulp_close(loss, cg.nn_utils.mse_np(x, t)[0], "small squares beside a large one")


def test_mse_criterion_formats(cg):
    rs = np.random.RandomState(8)
    x, t = rs.rand(4, 3, 32, 32).astype(np.float32), rs.rand(4, 3, 32, 32).astype(np.float32)
    ref_loss, ref_g = cg.nn_utils.mse_np(x, t)
    crit = cg.nn.MSECriterion()
    xi = cg.Tensor.from_numpy(x)                             # NHWC, as G's output
    tt = cg.Tensor.from_numpy(t, fmt="plain")                # NCHW
    assert xi.fmt == "nhwc" and tt.fmt == "plain"
    f = crit.forward(xi, tt)
    assert isinstance(f, cg.nn.LazyScalar) and crit.output is f
    gi = crit.backward(xi, tt)
    plain = cg.nn.MSECriterion()
    f_plain = plain.forward(cg.Tensor.from_numpy(x, fmt="plain"), tt)
    g_plain = plain.backward(cg.Tensor.from_numpy(x, fmt="plain"), tt)
    _ulp_close(float(f), float(f_plain), "NHWC against plain loss")
    _ulp_close(float(f), ref_loss, "loss")
    assert gi.fmt == "nhwc" and gi.shape == x.shape and g_plain.fmt == "plain"
    assert np.array_equal(gi.numpy(), ref_g) and np.array_equal(g_plain.numpy(), ref_g)
    # the gradient's memory is NHWC: element [n][h][w][c]
    assert np.array_equal(gi.t.cpu().numpy().reshape(4, 32, 32, 3), ref_g.transpose(0, 2, 3, 1))
    # buffers persist between calls
    p_loss, p_g = crit._loss.data_ptr(), gi.ptr
    f2 = crit.forward(xi, tt)
    assert crit._loss.data_ptr() == p_loss and crit.backward(xi, tt).ptr == p_g
    assert np.float32(float(f2)).tobytes() == np.float32(float(f)).tobytes()


# ------------------------------------------------------------------------------ the auto-encoder against torch
@pytest.mark.parametrize("dims,N", [((3, 32, 32), 4), ((1, 32, 32), 4), ((3, 64, 64), 2)])
def test_autoencoder_vs_torch(cg, dims, N):
    cg.manual_seed(13)
    AE = cg.models.create_G_autoencoder(dims, 100)
    _, G = AE.getParameters()
    enc, dec = AE.get(1), AE.get(2)
    x = np.random.RandomState(5).rand(N, *dims).astype(np.float32)
    snap = snapshot(AE)
    crit = cg.nn.MSECriterion()
    G.zero()
    xi = cg.nn.to_device(x)
    y = AE.forward(xi)
    assert not AE._planned_last and y.fmt == "nhwc"
    # PReLU's derivative jumps (1 or its weight, 0.25) where its input crosses zero.  The decoder's first Linear feeds one, and that
    # Linear's gradient has no sum to dilute an element in: gradWeight[i] = sum over the N = 2..4 rows of go[n][i] z[n], gradBias[i] =
    # sum_n go[n][i].  An element of h = lin(z) that fp32 rounding puts on the other side of zero than fp64 therefore moves a whole
    # row of both tensors fourfold, in any fp32 implementation (a torch fp32 run of the twin does it as well).  So the twin takes the
    # device's side for the elements of its own h that lie within KINK max|h| of zero, and the device's h must agree with the twin's
    # within that same distance (asserted below): every other element then has the twin's side on both.  With the side settled, the
    # per-tensor rule holds for every row of every tensor.
    lin, prelu = dec.modules[0], dec.modules[1]
    assert lin.typename == "nn.Linear" and prelu.typename == "nn.PReLU"
    h_dev = lin.output.numpy().copy()
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    params, taps = [], {}
    yt = torch_twin(AE, snap, xt, params, taps, sides={id(prelu): h_dev})
    loss = ((yt - xt.detach()) ** 2).mean()
    loss.backward()
    h_ref = taps[id(lin)].detach().numpy()
    near, flipped = taps["forced", id(prelu)]
    print(f"{near} of {h_ref.size} inputs of the decoder's first PReLU within {KINK:g} max|h| of zero, {flipped} of them on the other side on the device")
    assert np.abs(h_dev - h_ref).max() <= KINK * float(np.abs(h_ref).max()), "decoder Linear output"
    assert near <= 0.01 * h_ref.size
    f = crit.forward(y, xi)
    df = crit.backward(y, xi)
    assert df.fmt == "nhwc"
    gi = AE.backward(xi, df)
    close(cg.nn.as_plain(y).numpy(), yt.detach().numpy(), tol=1e-4, what="auto-encoder output")
    close(float(f), float(loss.detach()), tol=1e-4, what="loss")
    bulk_close(cg.nn.as_plain(gi).numpy(), xt.grad.numpy(), what="auto-encoder gradInput")
    # the encoder's output gradient = the gradInput of the decoder's first nn.Linear: what the nested walk must hand over
    assert lin.gradInput is not None and dec.gradInput is lin.gradInput
    gz, gz_ref = lin.gradInput.numpy(), taps[id(enc)].grad.numpy()
    assert gz.shape == (N, 100) and np.abs(gz).max() > 0 and np.abs(gz_ref).max() > 0
    bulk_close(gz, gz_ref, what="encoder output gradient")
    close(enc.output.numpy(), taps[id(enc)].detach().numpy(), tol=1e-4, what="code z")
    check_grads(G.numpy(), params)
    n_enc = cg.nn_utils.getNumberOfParameters(enc)
    assert np.abs(G.numpy()[:n_enc]).max() > 0, "the encoder received no gradient"
    nbn = 0
    for m in AE.listModules():
        if "BatchNormalization" in m.typename:
            rm, rv = taps[id(m)]
            close(m.running_mean.numpy(), rm.numpy(), tol=1e-4, what="running mean")
            close(m.running_var.numpy(), rv.numpy(), tol=1e-4, what="running var")
            nbn += 1
    assert nbn == 8


def test_fevalG_adam_step_vs_torch(cg):
    pg = importlib.import_module("pretrain_g")
    L2, CLAMP = 0.01, 1e-3            # weights reach sqrt(1/27) = 0.19: the penalty alone (0.01 p) passes the clamp on many of them
    cg.manual_seed(2)
    T = pg.GPretrainer(cg, (3, 32, 32), dict(seed=2, batchSize=4, G_L1=0.0, G_L2=L2, G_clamp=CLAMP, N_epoch=4, noiseDim=100))
    x = np.random.RandomState(9).rand(4, 3, 32, 32).astype(np.float32)
    snap = snapshot(T.G_AUTOENCODER)
    p0 = T.PARAMETERS_G_AUTOENCODER.numpy().copy()
    last = T.step(x)
    torch.cuda.synchronize()
    xt = torch.tensor(x, dtype=torch.float64)
    params, taps = [], {}
    yt = torch_twin(T.G_AUTOENCODER, snap, xt, params, taps)
    loss = ((yt - xt) ** 2).mean()
    loss.backward()
    gref = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    assert gref.size == p0.size
    close(float(last["f"]), float(loss.detach()), tol=1e-4, what="loss")
    raw = gref + L2 * p0
    assert (np.abs(raw) > CLAMP).sum() > 1000 and (np.abs(raw) < CLAMP).sum() > 1000, "the clamp must bite, and not everywhere"
    g = T.GRAD_PARAMETERS_G_AUTOENCODER.numpy().astype(np.float64)      # what fevalG handed to adam: penalty + clamp applied
    assert np.abs(g).max() <= np.float32(CLAMP)
    bulk_close(g, np.clip(raw, -CLAMP, CLAMP), what="clamped gradient")
    st = T.OPTSTATE["adam"]
    m, v = st["m"].numpy().astype(np.float64), st["v"].numpy().astype(np.float64)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=1e-4, atol=1e-20)     # (1 - beta2) g^2 rounded in fp32
    step = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (np.sqrt(v) + 1e-8)   # Torch7 adam: eps outside the bias correction
    np.testing.assert_allclose(T.PARAMETERS_G_AUTOENCODER.numpy(), p0 - step, rtol=0, atol=2e-7)


# ------------------------------------------------------------------------------ the scripts
ARGS = ["--synthetic", "--N_epoch", "64", "--batchSize", "16", "--epochs", "2", "--noplot"]


@pytest.fixture(scope="module")
def pretrained(cg, tmp_path_factory):
    """pretrain_g.py run twice with the same seed into the same directory: (directory, file name, bytes of run 1, bytes of run 2, the
    second run's trainer).  Both runs are pretrain_g.main() in this process, not two script processes: that also catches state that
    leaks from one run into the next (random streams, cached buffers), and the four tests below share the one pair of runs.  The
    price: a failure in here shows up as an error of each of them - read the fixture's traceback first."""
    pg = importlib.import_module("pretrain_g")
    d = tmp_path_factory.mktemp("g_pretrained")
    fn = pg.pretrained_filename(str(d), (3, 32, 32), 100)
    runs = []
    for _ in range(2):
        T = pg.main(ARGS + ["--save", str(d)])
        torch.cuda.synchronize()
        runs.append(open(fn, "rb").read())
        os.remove(fn)
    open(fn, "wb").write(runs[1])
    return d, fn, runs[0], runs[1], T


def test_seeded_pretraining_is_bit_reproducible(pretrained):
    _, _, a, b, T = pretrained
    assert len(a) > 4 * 5191687 and a == b
    assert T.EPOCH == 3


def test_saved_file_is_the_decoder(cg, pretrained):
    t7 = importlib.import_module("cat-generator_amd.t7")
    t7_nn = importlib.import_module("cat-generator_amd.t7_nn")
    _, fn, _, _, T = pretrained
    z = t7.load(fn)
    assert z["EPOCH"] == 3 and z["opt"]["noiseDim"] == 100 and z["opt"]["batchSize"] == 16      # the last save: EPOCH 2 + 1
    G = t7_nn.from_t7(z["G"])
    assert [repr(m) for m in G.modules] == [repr(m) for m in T.decoder.modules]
    n_enc = cg.nn_utils.getNumberOfParameters(T.encoder)
    assert np.array_equal(G.getParameters()[0].numpy(), T.PARAMETERS_G_AUTOENCODER.numpy()[n_enc:])


def test_train_starts_from_the_pretrained_decoder(cg, pretrained):
    tr = importlib.import_module("train")
    d, _, _, _, T = pretrained
    cg.manual_seed(1)
    D = cg.models.create_D((3, 32, 32))
    off = cg.tensor.rng().offset
    G = tr.load_pretrained_G(cg, str(d), (3, 32, 32), 100)
    assert G is not None and cg.tensor.rng().offset == off, "loading G must not move the random streams"
    S = cg.adversarial.State(dict(batchSize=16), G, D)          # what train.py does next: the flat vector before the first step
    n_enc = cg.nn_utils.getNumberOfParameters(T.encoder)
    assert np.array_equal(S.PARAMETERS_G.numpy(), T.PARAMETERS_G_AUTOENCODER.numpy()[n_enc:])
    bn_a = [m for m in G.listModules() if "BatchNormalization" in m.typename]
    bn_b = [m for m in T.decoder.listModules() if "BatchNormalization" in m.typename]
    assert len(bn_a) == len(bn_b) == 3
    for a, b in zip(bn_a, bn_b):
        assert np.array_equal(a.running_mean.numpy(), b.running_mean.numpy()) and np.array_equal(a.running_var.numpy(), b.running_var.numpy())
    assert all(m.train for m in G.listModules())
    assert tr.load_pretrained_G(cg, str(d), (1, 32, 32), 100) is None and tr.load_pretrained_G(cg, str(d), (3, 32, 32), 64) is None


def _run(args, timeout=420):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + args, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, f"{args[0]} exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def _saved(cg, path):
    """[G's flat parameters, D's flat parameters, every batch-norm running statistic] of an exported adversarial.net"""
    z = cg.checkpoint.import_t7(str(path))
    out = [z["G"].getParameters()[0].numpy(), z["D"].getParameters()[0].numpy()]
    for net in (z["G"], z["D"]):
        for m in net.listModules():
            if "BatchNormalization" in m.typename:
                out += [m.running_mean.numpy(), m.running_var.numpy()]
    return out


def test_pretrain_g_then_train_end_to_end(cg, pretrained, tmp_path):
    d = pretrained[0]
    common = ["train.py", "--synthetic", "--epochs", "1", "--N_epoch", "64", "--noplot", "--saveFreq", "1", "--V_dir", str(tmp_path / "nov")]
    out = _run(common + ["--G_pretrained_dir", str(d), "--save", str(tmp_path / "a")])
    assert "<trainer> loading pretrained G..." in out and "Number of free parameters in G: 5191687" in out
    empty = tmp_path / "empty"
    empty.mkdir()
    out_e = _run(common + ["--G_pretrained_dir", str(empty), "--save", str(tmp_path / "b")])
    out_n = _run(common + ["--save", str(tmp_path / "c")])
    assert "loading pretrained G" not in out_e and "loading pretrained G" not in out_n
    a, b, c = (_saved(cg, tmp_path / k / "adversarial.net") for k in "abc")
    for u, v in zip(b, c):
        assert np.array_equal(u, v), "a run pointed at an empty directory differs from a run without the flag"
    assert not np.array_equal(a[0], b[0]), "the run that loaded the pretrained G must differ from the fresh one"
