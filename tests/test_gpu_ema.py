"""--G_ema on the device: the running average of G's weights kept inside its optimiser step.

Kernels (csrc/optim.hip adam_ema_k / ema_k) through the C ABI over their dispatch edges - a float4 body with a live scalar tail, the
all-scalar twin behind any pointer 4 bytes off a 16-byte boundary, the grid-stride wrap behind cg::ew_grid's cap - with two measures:
  bits_equal      the fused entry against cg_adam_step (p, g, m, v) and against cg_ema_update on its p' (e); the device-counter forms
                  against the host-count forms
  rounding_close  e against the fp64 restatement optim.ema_np on the p' read back from the device and the fp32 decay:
                  |d| <= r 2^-24 (d |e| + (1 - d) |p'|), r = 5: the roundings of 1 - d, of the product and of the fma, plus 2
Then the trainer: the flag changes nothing but e, replay and resume reproduce e bit for bit, export / import / sample.py / train.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from helpers import bits_equal, dev, edge_normal, host, rounding_close

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
R_EMA = 5                                     # 1 - d, the product, the fma: 3 roundings, + 2
D_WARM, D_CAP = float(f32(2.0 / 11.0)), float(f32(0.999))          # d_1 (where 1 - d does round) and the capped decay
SETTINGS = [(0.0, 0.0, 5.0, 1), (1e-4, 1e-4, 1.0, 1)]               # (l1, l2, clamp, write_back): G's own, and one with the penalty live


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    p, g, e = (edge_normal(rng, (n, 1)).ravel() for _ in range(3))
    m, v = (rng.standard_normal(n) * 0.1).astype(f32), (rng.random(n) * 0.1).astype(f32)      # v >= 0
    return p, g, m, v, e


def ptr(t):
    return t.data_ptr()


def ema_close(e_new, e_old, p_new, d, what):
    optim = importlib.import_module("cat-generator_amd.optim")
    terms = d * np.abs(e_old.astype(f64)) + (1.0 - d) * np.abs(p_new.astype(f64))
    return rounding_close(e_new, optim.ema_np(e_old, p_new, d), terms, R_EMA, what)


# ------------------------------------------------------------------------------ 1. dispatch edges
# 1 048 576 + 1024 + 3: 262 400 float4 lanes against the 262 144 of cg::ew_grid's cap - the vector kernel's stride wraps - and a tail of 3
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1027, 1048576 + 1024 + 3])
def test_fused_step_over_the_dispatch_edges(cg, n):
    L, st = cg.lib(), cg.tensor.stream()
    p0, g0, m0, v0, e0 = inputs(n, n)
    for t in (1, 3):
        for l1, l2, clamp, wb in SETTINGS:
            ref = [dev(a) for a in (p0, g0, m0, v0)]
            L.adam_step(st, *map(ptr, ref), n, LR, B1, B2, EPS, t, l1, l2, clamp, wb)
            want = [host(a) for a in ref]
            for d in (D_WARM, D_CAP):
                # the stand-alone kernel on that p': aligned, and behind either pointer off its boundary - the same bits
                es = []
                for mis in ((False, False), (True, False), (False, True)):
                    pe, pp = dev(e0, mis[0]), dev(want[0], mis[1])
                    L.ema_update(st, ptr(pe), ptr(pp), n, d)
                    es.append(host(pe))
                    bits_equal(host(pp), want[0], f"cg_ema_update left p alone, n = {n}")
                    bits_equal(es[-1], es[0], f"cg_ema_update e, n = {n}, (e, p) off alignment = {mis}")
                ema_close(es[0], e0, want[0], d, f"cg_ema_update vs fp64, n = {n}, t = {t}, d = {d:.6f}")
                # the fused entry: all five buffers aligned, and each one of them 4 bytes off
                for off in (None, 0, 1, 2, 3, 4):
                    bufs = [dev(a, k == off) for k, a in enumerate((p0, g0, m0, v0, e0))]
                    L.adam_step_ema(st, *map(ptr, bufs), n, LR, B1, B2, EPS, t, l1, l2, clamp, wb, d)
                    what = f"n = {n}, t = {t}, (l1, l2, clamp) = {(l1, l2, clamp)}, d = {d:.6f}, buffer off alignment: {off}"
                    for name, a, b in zip("pgmv", bufs, want):
                        bits_equal(host(a), b, f"cg_adam_step_ema {name} vs cg_adam_step, {what}")
                    bits_equal(host(bufs[4]), es[0], f"cg_adam_step_ema e vs cg_ema_update, {what}")


# ------------------------------------------------------------------------------ 2. counter forms
@pytest.mark.parametrize("count", [1, 2, 9, 8990, 8991])
def test_device_counter_forms_match_the_host_count(cg, count):
    L, st = cg.lib(), cg.tensor.stream()
    n, D = 1027, 0.999
    p0, g0, m0, v0, e0 = inputs(n, 77)
    nd = torch.tensor([count], dtype=torch.int64, device="cuda")
    d = cg.optim.ema_decay(D, count)
    a, b = dev(e0), dev(e0)
    pp = dev(p0)
    L.ema_update(st, ptr(a), ptr(pp), n, d)
    L.ema_update_dev(st, ptr(b), ptr(pp), n, float(f32(D)), ptr(nd))
    bits_equal(host(b), host(a), f"cg_ema_update_dev vs cg_ema_update, n = {count}")
    t = count                                                     # the matching t, read from a counter of its own
    td = torch.tensor([t], dtype=torch.int64, device="cuda")
    l1, l2, clamp, wb = SETTINGS[0]
    A, B = [dev(x) for x in (p0, g0, m0, v0, e0)], [dev(x) for x in (p0, g0, m0, v0, e0)]
    L.adam_step_ema(st, *map(ptr, A), n, LR, B1, B2, EPS, t, l1, l2, clamp, wb, d)
    L.adam_step_ema_dev(st, *map(ptr, B), n, LR, B1, B2, EPS, ptr(td), l1, l2, clamp, wb, float(f32(D)), ptr(nd))
    for name, x, y in zip("pgmve", B, A):
        bits_equal(host(x), host(y), f"cg_adam_step_ema_dev {name} vs cg_adam_step_ema, n = t = {count}")
    assert int(nd.item()) == count and int(td.item()) == t          # the kernels read the counters, the host advances them


# ------------------------------------------------------------------------------ 3. recurrence
def test_twelve_updates_through_the_device_counter(cg):
    """Each step's e against fp64 from the device's previous e and that step's p': the error of one step, never an accumulated one."""
    L, st = cg.lib(), cg.tensor.stream()
    n, D = 1027, 0.999
    p0, _, m0, v0, e0 = inputs(n, 5)
    p, m, v, e = dev(p0), dev(np.zeros(n, f32)), dev(np.zeros(n, f32)), dev(p0)         # e0 = p0, as State starts it
    td, nd = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    rng = np.random.default_rng(9)
    e_prev = host(e)
    for k in range(1, 13):
        g = dev(edge_normal(rng, (n, 1)).ravel())
        L.counter_add(st, ptr(td), 1)
        L.counter_add(st, ptr(nd), 1)
        L.adam_step_ema_dev(st, ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, LR, B1, B2, EPS, ptr(td), 0.0, 0.0, 5.0, 1, float(f32(D)), ptr(nd))
        host(g)
        e_now, p_now = host(e), host(p)
        ema_close(e_now, e_prev, p_now, cg.optim.ema_decay(D, k), f"update {k} of 12")
        e_prev = e_now
    assert int(nd.item()) == 12 and int(td.item()) == 12


# ------------------------------------------------------------------------------ 4. the trainer
def make_state(cg, px, seed, **opt):
    cg.manual_seed(seed)
    dims = (3, px, px)
    G, D = cg.models.create_G(dims, 100), cg.models.create_D(dims)
    return cg.adversarial.State(dict(batchSize=8, scale=px, seed=4, **opt), G, D)


def make_data(cg, px):
    return cg.adversarial.TrainData(np.random.RandomState(10).rand(32, 3, px, px).astype(f32))


def opt_tensors(cg, S):
    """every tensor of the optimiser state (Adam's m and v of both nets, momentum buffers, variances) by name"""
    out = {}
    for method, per_net in S.OPTSTATE.items():
        for net, stt in per_net.items():
            for k, v in stt.items():
                if isinstance(v, cg.tensor.Tensor):
                    out[f"{method}/{net}/{k}"] = v.numpy()
    return out


@pytest.mark.parametrize("px,method", [(32, "adam"), (16, "sgd")])
def test_the_flag_moves_nothing_but_the_average(cg, px, method):
    """Two runs from the same seed, one with G_ema: parameters, optimiser state and the counter stream's position stay bit for bit
    what they are without it; e follows the fp64 recurrence over G's snapshots step by step; the averaged net's storage is e.  At
    16 px with --G_optmethod sgd the average moves in the stand-alone kernel behind the step."""
    def run(**opt):
        S = make_state(cg, px, 21, G_optmethod=method, **opt)
        data = make_data(cg, px)
        snaps = [(S.PARAMETERS_G.numpy(), S.PARAMETERS_G_EMA.numpy() if S.EMA else None)]
        for k in range(3):
            cg.lib().trace = [] if k == 2 else None          # the entry points the third iteration calls, in order
            cg.adversarial.iteration(S, data, 8)
            calls, cg.lib().trace = cg.lib().trace, None
            snaps.append((S.PARAMETERS_G.numpy(), S.PARAMETERS_G_EMA.numpy() if S.EMA else None))
        torch.cuda.synchronize()
        return S, snaps, cg.tensor.rng().offset, [name for name, _ in calls]
    A, snapsA, offA, callsA = run(G_ema=0.999)
    B, snapsB, offB, callsB = run()
    # the launches: without the flag none of the new entry points; with it G's cg_adam_step becomes cg_adam_step_ema (one call for
    # one), or cg_ema_update follows G's cg_sgd_step - and nothing else in the iteration changes
    assert not [c for c in callsB if "ema" in c]
    if method == "adam":
        assert callsB.count("cg_adam_step") == 2 and callsA.count("cg_adam_step") == 1 and callsA.count("cg_adam_step_ema") == 1
        assert [("cg_adam_step" if c == "cg_adam_step_ema" else c) for c in callsA] == callsB
    else:
        assert callsA.count("cg_ema_update") == 1 and callsA[callsA.index("cg_ema_update") - 1] == "cg_sgd_step"
        assert [c for c in callsA if c != "cg_ema_update"] == callsB
    assert not hasattr(B, "MODEL_G_EMA") and "G_ema" not in B.OPT
    bits_equal(A.PARAMETERS_G.numpy(), B.PARAMETERS_G.numpy(), "PARAMETERS_G with and without the flag")
    bits_equal(A.PARAMETERS_D.numpy(), B.PARAMETERS_D.numpy(), "PARAMETERS_D with and without the flag")
    ta, tb = opt_tensors(cg, A), opt_tensors(cg, B)
    assert ta.keys() == tb.keys() and {"adam/D/m", "adam/D/v"} <= ta.keys() and (method != "adam" or {"adam/G/m", "adam/G/v"} <= ta.keys())
    for k in ta:
        bits_equal(ta[k], tb[k], f"optimiser state {k} with and without the flag")
    assert offA == offB, "the flag moved the counter stream"
    assert A.ema_n() == 3
    bits_equal(snapsA[0][1], snapsA[0][0], "e starts as a copy of PARAMETERS_G")
    for k in range(1, 4):
        assert not np.array_equal(snapsA[k][0], snapsA[k - 1][0]), "G did not move"
        ema_close(snapsA[k][1], snapsA[k - 1][1], snapsA[k][0], cg.optim.ema_decay(0.999, k), f"{px} px {method}: e after update {k}")
    first = A.MODEL_G_EMA.parameters()[0][0]
    assert first.ptr == A.PARAMETERS_G_EMA.ptr == A.EMA["e"].ptr, "MODEL_G_EMA's parameters are not views into e"
    assert all(not m.train for m in A.MODEL_G_EMA.listModules()), "MODEL_G_EMA left evaluate mode"


# ------------------------------------------------------------------------------ 5. replay
def test_graph_replay_reproduces_the_average(cg):
    """2 eager + 1 replayed iteration through GraphedIteration against 3 eager ones with the same device-side counters: e and n bit for bit."""
    def run(graph):
        S = make_state(cg, 32, 41, G_ema=0.999)
        data = make_data(cg, 32)
        if graph:
            it = cg.adversarial.GraphedIteration(S, data, 8, warmup=2)
            it()
        else:
            S.device_rng = True
            for k in ("D", "G"):
                S.OPTSTATE["adam"][k]["device_step"] = True
            r = cg.tensor.rng(); r.enable_device_base()
            for _ in range(3):
                off0 = r.offset
                cg.adversarial.iteration(S, data, 8)
                cg.lib().counter_add(cg.tensor.stream(), r.dev_base.data_ptr(), r.offset - off0)
                r.offset = off0
        torch.cuda.synchronize()
        assert S.EMA["n"] == int(S.EMA["n_dev"].item()), "the host count of averaged updates drifted from the device's"
        return S.PARAMETERS_G_EMA.numpy(), S.ema_n(), S.PARAMETERS_G.numpy()
    ge, gn, gp = run(True)
    ee, en, ep = run(False)
    assert gn == en == 3
    bits_equal(gp, ep, "PARAMETERS_G, replay vs eager")
    bits_equal(ge, ee, "e, replay vs eager")
    assert not np.array_equal(ge, gp)


# ------------------------------------------------------------------------------ 6. resume and export
# what checkpoint.save writes for a 32 px run without the flag after Adam has stepped: the key set before --G_ema existed
PARENT_KEYS = sorted(
    ["EPOCH", "OPT", "PARAMETERS_D", "PARAMETERS_G", "rng", "host_random_keys", "host_random_meta", "dataset_random_keys", "dataset_random_meta"]
    + [f"bnG{i}_{s}" for i in range(3) for s in ("mean", "var")]
    + [f"opt/adam/{net}/{k}" for net in "DG" for k in "tmv"]
    + [f"opt/{m}/{net}/learningRate" for m in ("adagrad", "sgd") for net in "DG"] + [f"opt/sgd/{net}/momentum" for net in "DG"])


def test_resume_continues_the_average_bit_for_bit(cg, tmp_path):
    data = make_data(cg, 32)
    A = make_state(cg, 32, 72, G_ema=0.999)
    for _ in range(2):
        cg.adversarial.iteration(A, data, 8)
    ck = cg.checkpoint.save(str(tmp_path / "a.npz"), A)
    z = np.load(ck)
    assert sorted(z.files) == sorted(PARENT_KEYS + ["PARAMETERS_G_ema", "G_ema_n"]) and int(z["G_ema_n"]) == 2
    for _ in range(2):
        cg.adversarial.iteration(A, data, 8)
    B = make_state(cg, 32, 72, G_ema=0.999)
    cg.checkpoint.load(ck, B)
    assert B.ema_n() == 2
    for _ in range(2):
        cg.adversarial.iteration(B, data, 8)
    torch.cuda.synchronize()
    assert A.ema_n() == B.ema_n() == 4
    bits_equal(B.PARAMETERS_G.numpy(), A.PARAMETERS_G.numpy(), "PARAMETERS_G after the resume")
    bits_equal(B.PARAMETERS_G_EMA.numpy(), A.PARAMETERS_G_EMA.numpy(), "e after the resume")


def test_checkpoints_without_the_flag_and_across_it(cg, tmp_path, capsys):
    data = make_data(cg, 32)
    off = make_state(cg, 32, 72)
    cg.adversarial.iteration(off, data, 8)
    ck_off = cg.checkpoint.save(str(tmp_path / "off.npz"), off)
    assert sorted(np.load(ck_off).files) == PARENT_KEYS, "a run without the flag writes another key set than before"
    on = make_state(cg, 32, 72, G_ema=0.999)
    cg.adversarial.iteration(on, data, 8)
    ck_on = cg.checkpoint.save(str(tmp_path / "on.npz"), on)
    # the flag on, a file without the average: e starts from the loaded p with n = 0, and the load says so
    C = make_state(cg, 32, 73, G_ema=0.999)
    capsys.readouterr()
    cg.checkpoint.load(ck_off, C)
    assert "holds no averaged generator" in capsys.readouterr().out and C.ema_n() == 0
    bits_equal(C.PARAMETERS_G_EMA.numpy(), off.PARAMETERS_G.numpy(), "e restarted from the loaded G")
    # the flag off, a file with the average: ignored
    E = make_state(cg, 32, 73)
    cg.checkpoint.load(ck_on, E)
    assert E.EMA is None and not hasattr(E, "MODEL_G_EMA")
    bits_equal(E.PARAMETERS_G.numpy(), on.PARAMETERS_G.numpy(), "PARAMETERS_G of the loaded file")


def _sample_options(monkeypatch, save, base, *flags):
    monkeypatch.syspath_prepend(ROOT)
    sample = importlib.import_module("sample")
    monkeypatch.setattr(sys, "argv", ["sample.py", "--save", str(save), "--G_base", base, "--D_base", base, "--batchSize", "8", *flags])
    return sample, sample.parse()


def test_export_import_and_sampling_from_the_average(cg, tmp_path, monkeypatch):
    data = make_data(cg, 32)
    S = make_state(cg, 32, 33, G_ema=0.999)
    for _ in range(2):
        cg.adversarial.iteration(S, data, 8)
    net = cg.checkpoint.export_t7(str(tmp_path / "adversarial.net"), S)
    npz = cg.checkpoint.save(str(tmp_path / "adversarial.npz"), S)
    e = S.PARAMETERS_G_EMA.numpy()
    assert not np.array_equal(e, S.PARAMETERS_G.numpy())
    noise = np.random.RandomState(3).uniform(-1, 1, (8, 100)).astype(f32)
    want = cg.nn.as_nhwc(S.sync_ema_stats().forward(cg.nn.to_device(noise))).numpy()
    z = cg.checkpoint.import_t7(net)
    assert int(z["G_ema_n"]) == 2
    Ge = z["G_ema"]
    Ge.evaluate()
    bits_equal(cg.nn.as_nhwc(Ge.forward(cg.nn.to_device(noise))).numpy(), want, "the imported G_ema net vs MODEL_G_EMA on 8 noise rows")
    # sample.py --G_ema: from the .net and from the .npz, a generator whose flat parameters are the file's averaged vector
    for base in ("adversarial.net", "adversarial.npz"):
        sample, o = _sample_options(monkeypatch, tmp_path, base, "--G_ema")
        G, _ = sample.load_models(cg, o, (3, 32, 32))
        bits_equal(G.getParameters()[0].numpy(), e, f"sample.py --G_ema from {base}")
        assert all(not m.train for m in G.listModules())
        sample, o = _sample_options(monkeypatch, tmp_path, base)
        G, _ = sample.load_models(cg, o, (3, 32, 32))
        bits_equal(G.getParameters()[0].numpy(), S.PARAMETERS_G.numpy(), f"sample.py without the flag from {base}")
    # a run without the flag: no G_ema field, and sample.py --G_ema says what is missing
    off = make_state(cg, 32, 33)
    cg.adversarial.iteration(off, data, 8)
    plain = tmp_path / "plain"
    plain.mkdir()
    z = cg.checkpoint.import_t7(cg.checkpoint.export_t7(str(plain / "adversarial.net"), off))
    assert "G_ema" not in z and "G_ema_n" not in z
    cg.checkpoint.save(str(plain / "adversarial.npz"), off)
    for base in ("adversarial.net", "adversarial.npz"):
        sample, o = _sample_options(monkeypatch, plain, base, "--G_ema")
        with pytest.raises(ValueError, match="holds no averaged generator"):
            sample.load_models(cg, o, (3, 32, 32))


# ------------------------------------------------------------------------------ 7. front end
def test_train_py_writes_the_averaged_grid_and_checkpoint(cg, tmp_path, monkeypatch):
    """One epoch of train.py --G_ema.  --saveFreq 1 makes the one epoch save (at the default 30 it would not), --V_dir and
    --G_pretrained_dir keep a stray logs/ directory out.  N_epoch 16 at batch 8 is 4 iterations (adversarial.train steps by half a
    batch: 8, 8, 8 and 4 images), so the stored count of averaged updates is G's Adam step count, 4."""
    from PIL import Image
    monkeypatch.syspath_prepend(ROOT)
    train = importlib.import_module("train")
    tmp = str(tmp_path / "logs")
    train.main(["--synthetic", "--batchSize", "8", "--N_epoch", "16", "--epochs", "1", "--G_ema", "0.999", "--save", tmp, "--saveFreq", "1",
                "--V_dir", str(tmp_path / "nov"), "--G_pretrained_dir", str(tmp_path / "nog")])
    sizes = {}
    for sub in ("images", "images_ema"):
        files = sorted(os.listdir(os.path.join(tmp, sub)))
        assert len(files) == 1 and files[0].endswith(".png"), (sub, files)
        sizes[sub] = Image.open(os.path.join(tmp, sub, files[0])).size
    assert sizes["images_ema"] == sizes["images"]
    z = np.load(os.path.join(tmp, "adversarial.npz"))
    assert "PARAMETERS_G_ema" in z.files and int(z["G_ema_n"]) == int(z["opt/adam/G/t"]) == 4
    assert z["PARAMETERS_G_ema"].shape == z["PARAMETERS_G"].shape and not np.array_equal(z["PARAMETERS_G_ema"], z["PARAMETERS_G"])
    assert "G_ema" in cg.checkpoint.import_t7(os.path.join(tmp, "adversarial.net"))
