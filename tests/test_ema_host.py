"""--G_ema without a GPU: the four entry points in the parsed header and in the library, their argument checks (every refusal happens
before a launch), the warm-up schedule optim.ema_decay, train.py's flag, and a State without the flag being what it always was."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

ADAM = [("void*", "stream"), ("float*", "p"), ("float*", "g"), ("float*", "m"), ("float*", "v"), ("float*", "e"), ("long", "n"),
        ("float", "lr"), ("float", "beta1"), ("float", "beta2"), ("float", "eps")]
TAIL = [("float", "l1"), ("float", "l2"), ("float", "clamp"), ("int", "write_back_grad")]
PROTOS = {
    "cg_ema_update": ("int", [("void*", "stream"), ("float*", "e"), ("const float*", "p"), ("long", "n"), ("float", "decay")]),
    "cg_ema_update_dev": ("int", [("void*", "stream"), ("float*", "e"), ("const float*", "p"), ("long", "n"), ("float", "decay_cap"),
                                  ("const uint64_t*", "n_dev")]),
    "cg_adam_step_ema": ("int", ADAM + [("int", "t")] + TAIL + [("float", "decay")]),
    "cg_adam_step_ema_dev": ("int", ADAM + [("const uint64_t*", "t_dev")] + TAIL + [("float", "decay_cap"), ("const uint64_t*", "n_dev")]),
}


@pytest.fixture(scope="module")
def cg():
    return importlib.import_module("cat-generator_amd")


def test_the_four_prototypes_are_declared_and_exported(cg):
    abi = importlib.import_module("cat-generator_amd._abi")
    protos = abi.parse_header()
    dll = ctypes.CDLL(abi.LIB_PATH)
    for name, want in PROTOS.items():
        assert protos.get(name) == want, (name, protos.get(name))
        assert hasattr(dll, name), f"{name} declared in include/catgan.h but not exported"


P = 4096        # any non-null address: every call below is refused before a kernel could be launched


def _calls(L, decay, null=None):
    """name -> a call with `decay` and, at position `null` of its pointers, a null pointer"""
    def ptrs(k):
        return [None if i == null else P for i in range(k)]
    a = (1e-3, 0.9, 0.999, 1e-8)
    return {
        "cg_ema_update": lambda: L.ema_update(None, *ptrs(2), 8, decay),
        "cg_ema_update_dev": lambda: (lambda q: L.ema_update_dev(None, q[0], q[1], 8, decay, q[2]))(ptrs(3)),
        "cg_adam_step_ema": lambda: L.adam_step_ema(None, *ptrs(5), 8, *a, 1, 0.0, 0.0, 5.0, 1, decay),
        "cg_adam_step_ema_dev": lambda: (lambda q: L.adam_step_ema_dev(None, *q[:5], 8, *a, q[5], 0.0, 0.0, 5.0, 1, decay, q[6]))(ptrs(7)),
    }


@pytest.mark.parametrize("name,npointers", [("cg_ema_update", 2), ("cg_ema_update_dev", 3), ("cg_adam_step_ema", 5),
                                            ("cg_adam_step_ema_dev", 7)])
def test_bad_arguments_are_refused_by_name(cg, name, npointers):
    L = cg.lib()
    for k in range(npointers):
        with pytest.raises(cg.CatganError, match=name + ": null pointer"):
            _calls(L, 0.5, null=k)[name]()
    for decay in (0.0, 1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(cg.CatganError, match=name + ": decay"):
            _calls(L, decay)[name]()


def test_a_step_count_below_one_is_refused(cg):
    with pytest.raises(cg.CatganError, match="cg_adam_step_ema: step count"):
        cg.lib().adam_step_ema(None, P, P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 0, 0.0, 0.0, 5.0, 1, 0.5)


def test_warm_up_schedule(cg):
    """d_n = (float) min((double)(float)D, (1 + n) / (10 + n)): 2/11 at n = 1, growing until D = 0.999 caps it - first at n = 8991,
    since 8991/9000 = 0.99900 lies below (float)0.999 = 0.99900001287... and 8992/9001 above it."""
    d = {n: cg.optim.ema_decay(0.999, n) for n in (1, 2, 9, 8990, 8991, 10 ** 6)}
    for n, v in d.items():
        assert isinstance(v, float) and float(f32(v)) == v, n                  # a Python float holding an fp32 value
    assert d[1] == float(f32(2.0 / 11.0))
    assert d[1] < d[2] < d[9] < d[8990]
    assert d[8990] == float(f32(8991.0 / 9000.0))       # the last uncapped one: below the cap in double, the cap itself once rounded to fp32
    assert d[8991] == d[10 ** 6] == float(f32(0.999))
    assert 8991.0 / 9000.0 < float(f32(0.999)) < 8992.0 / 9001.0
    # the fp64 restatement: d e + (1 - d) p with the fp32 d
    e, p = np.array([1.0, -2.0], f32), np.array([3.0, 0.5], f32)
    np.testing.assert_array_equal(cg.optim.ema_np(e, p, d[1]), d[1] * e.astype(np.float64) + (1.0 - d[1]) * p.astype(np.float64))


def test_train_parser_takes_and_validates_the_flag(monkeypatch, capsys):
    monkeypatch.syspath_prepend(ROOT)
    train = importlib.import_module("train")
    assert train.parse(["--G_ema", "0.999"]).G_ema == 0.999
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(SystemExit):
            train.parse(["--G_ema=" + bad])
        assert "--G_ema" in capsys.readouterr().err
    # off - by default or by an explicit 0 - the parsed options are those of a command line without the flag
    assert vars(train.parse(["--G_ema", "0"])) == vars(train.parse([])) and "G_ema" not in vars(train.parse([]))


def test_state_without_the_flag_is_unchanged(cg):
    cg.manual_seed(5)
    dims = (3, 16, 16)
    S = cg.adversarial.State(dict(batchSize=8, scale=16), cg.models.create_G(dims, 100), cg.models.create_D(dims))
    assert not hasattr(S, "MODEL_G_EMA") and S.EMA is None
    want = dict(cg.adversarial.DEFAULT_OPT, batchSize=8, scale=16)
    assert S.OPT == want and "G_ema" not in S.OPT and "G_ema" not in cg.adversarial.DEFAULT_OPT
    with pytest.raises(ValueError, match="G_ema"):
        cg.adversarial.State(dict(batchSize=8, scale=16, G_ema=1.0), cg.models.create_G(dims, 100), cg.models.create_D(dims))
