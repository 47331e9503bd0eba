"""CPU-side checks of the generator pre-training (no GPU): the two nn.MSECriterion entry points are declared, exported and refuse bad
arguments; the encoder / auto-encoder have the reference's structure, parameter counts (against a torch.nn twin built here) and
weight-init scoping; nn_utils.mse_np gives hand-computed answers; pretrain_g.py's flags are the Lua ones and its file name is the one
train.py --G_pretrained_dir looks for."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def cg():
    return importlib.import_module("cat-generator_amd")


def test_mse_entry_points_declared_and_exported(cg):
    abi = importlib.import_module("cat-generator_amd._abi")
    protos = abi.parse_header()
    sig = ("int", [("void*", "stream"), ("const float*", "x"), ("const float*", "t"), ("float*", "loss"), ("long", "n")])
    assert protos["cg_mse_forward"] == sig
    assert protos["cg_mse_backward"] == ("int", sig[1][:3] + [("float*", "dx"), ("long", "n")])
    dll = ctypes.CDLL(abi.LIB_PATH)
    assert hasattr(dll, "cg_mse_forward") and hasattr(dll, "cg_mse_backward")
    assert cg.lib().abi_version() == 2


def test_mse_bad_arguments_raise(cg):
    L = cg.lib()
    for fn in (L.mse_forward, L.mse_backward):
        for args in ((None, None, 16, 16, 4), (None, 16, None, 16, 4), (None, 16, 16, None, 4)):
            with pytest.raises(cg.CatganError, match="null pointer"):
                fn(*args)
        for n in (0, -1):
            with pytest.raises(cg.CatganError, match="bad length"):
                fn(None, 16, 16, 16, n)


ENCODER = ["nn.SpatialConvolution", "nn.SpatialBatchNormalization", "nn.LeakyReLU", "nn.SpatialMaxPooling"] * 3 + \
          ["nn.SpatialConvolution", "nn.SpatialBatchNormalization", "nn.LeakyReLU",
           "nn.View", "nn.Linear", "nn.BatchNormalization", "nn.LeakyReLU", "nn.Linear"]          # models.lua:54-78


def _torch_encoder(C, H, W, noiseDim):
    """models.lua:50-83 in torch.nn, for its parameter count."""
    T = torch.nn
    feat = 32 * (H // 8) * (W // 8)
    blocks = []
    for i, (a, b) in enumerate(((C, 16), (16, 16), (16, 32), (32, 32))):
        blocks += [T.Conv2d(a, b, 3, padding=1), T.BatchNorm2d(b), T.LeakyReLU(0.333)] + ([T.MaxPool2d(2)] if i < 3 else [])
    return T.Sequential(*blocks, T.Flatten(), T.Linear(feat, 1024), T.BatchNorm1d(1024), T.LeakyReLU(0.333), T.Linear(1024, noiseDim))


@pytest.mark.parametrize("dims,count", [((3, 32, 32), 646708), ((1, 32, 32), 646420), ((3, 64, 64), None)])
def test_encoder_structure_and_parameter_count(cg, dims, count):
    cg.manual_seed(1)
    E = cg.models.create_G_encoder32(dims, 100)
    assert [m.typename for m in E.modules] == ENCODER
    convs = [m for m in E.modules if m.typename == "nn.SpatialConvolution"]
    assert [(m.nInputPlane, m.nOutputPlane, m.kW, m.kH, m.padW, m.padH) for m in convs] == \
        [(dims[0], 16, 3, 3, 1, 1), (16, 16, 3, 3, 1, 1), (16, 32, 3, 3, 1, 1), (32, 32, 3, 3, 1, 1)]
    feat = 32 * dims[1] * dims[2] // 64
    assert E.modules[15].sizes == (feat,) and E.modules[16].weight.shape == (1024, feat) and E.modules[19].weight.shape == (100, 1024)
    assert all(m.negative_scale == 0.333 for m in E.modules if m.typename == "nn.LeakyReLU")
    twin = sum(p.numel() for p in _torch_encoder(*dims, 100).parameters())
    assert cg.nn_utils.getNumberOfParameters(E) == twin
    if count is not None:
        assert twin == count


def test_autoencoder_is_encoder_plus_create_G(cg):
    cg.manual_seed(1)
    A = cg.models.create_G_autoencoder((3, 32, 32), 100)
    assert A.typename == "nn.Sequential" and A.size() == 2
    enc, dec = A.get(1), A.get(2)
    assert [m.typename for m in enc.modules] == ENCODER
    G = cg.models.create_G((3, 32, 32), 100)
    assert [repr(m) for m in dec.modules] == [repr(m) for m in G.modules]
    n = cg.nn_utils.getNumberOfParameters
    assert n(G) == 5191687 and n(A) == n(enc) + n(G) == 646708 + 5191687
    flat, grad = A.getParameters()                       # encoder first, then the decoder: one vector
    assert flat.nElement() == grad.nElement() == n(A)
    A64 = cg.models.create_G_autoencoder((3, 64, 64), 100)
    assert A64.get(2).modules[0].weight.shape == (512 * 8 * 8, 100)          # the 64x64 decoder, as create_G picks it
    assert n(A64) == n(A64.get(1)) + n(cg.models.create_G((3, 64, 64), 100))
    with pytest.raises(NotImplementedError):
        cg.models.create_G_autoencoder((3, 16, 16), 100)


def test_encoder_weight_init_scoping_matches_G(cg):
    """weight-init.lua:52-71 on the encoder, as on G: every top-level convolution / Linear is re-drawn from U(+-sqrt(1 / fan_in)) (the
    heuristic's sqrt(1 / (3 fan_in)) times reset's sqrt(3)), and every top-level bias - the batch norms' included - is zeroed."""
    cg.manual_seed(5)
    E = cg.models.create_G_encoder32((3, 32, 32), 100)
    G = cg.models.create_G((3, 32, 32), 100)
    for net in (E, G):
        for m in net.modules:
            if getattr(m, "bias", None) is not None:
                assert np.all(m.bias.numpy() == 0), f"{m}: bias not zeroed"
            if m.typename in ("nn.SpatialConvolution", "cudnn.SpatialConvolution", "nn.Linear"):
                fan_in = m.weight.nElement() // m.weight.shape[0]
                w = m.weight.numpy()
                bound = np.sqrt(1.0 / fan_in)
                assert np.abs(w).max() <= bound * (1 + 1e-6)
                if w.size >= 400 and m.typename != "cudnn.SpatialConvolution":    # the draw fills the range (cudnn.* is not re-drawn: :56 names nn.*)
                    assert np.abs(w).max() >= 0.9 * bound


def test_mse_np_known_answers(cg):
    mse = cg.nn_utils.mse_np
    loss, g = mse([1, 2, 3], [1, 2, 5])                      # (0 + 0 + 4) / 3
    assert loss == np.float32(4.0 / 3.0) and loss.dtype == np.float32
    assert np.array_equal(g, np.array([0, 0, np.float32(2.0) / np.float32(3.0) * np.float32(-2.0)], np.float32)) and g.dtype == np.float32
    loss, g = mse(np.full((2, 2), 0.5), np.zeros((2, 2)))    # 4 * 0.25 / 4 ; 2/4 * 0.5
    assert loss == np.float32(0.25) and np.array_equal(g, np.full((2, 2), 0.25, np.float32))
    loss, g = mse([3.0], [1.0])                              # n = 1: (2)^2, 2 * 2
    assert loss == 4.0 and g[0] == 4.0
    x = np.arange(8, dtype=np.float32)
    loss, g = mse(x, x)
    assert loss == 0.0 and not g.any()
    # the difference is rounded to fp32 BEFORE it is squared: 1 + 2^-24 is 1 in fp32, so the inputs are equal
    loss, _ = mse(np.array([1.0 + 2.0 ** -24]), np.array([1.0]))
    assert loss == 0.0
    # fp64 accumulation: 4096 squares of 1e-3 beside one of 1e4 are not lost (fp32 accumulation would drop each 1e-6 against 1e8)
    d = np.full(4097, 1e-3, np.float32)
    d[0] = 1e4
    loss, _ = mse(d, np.zeros_like(d))
    exact = (float(np.float32(1e4)) ** 2 + 4096 * float(np.float32(1e-3)) ** 2) / 4097
    assert loss == np.float32(exact)


def test_pretrain_g_flag_defaults_are_the_lua_ones():
    pg = importlib.import_module("pretrain_g")
    o = pg.parse([])
    lua = dict(save="logs", batchSize=16, noplot=False, window=23, seed=1, aws=False, saveFreq=1, gpu=0, threads=8, colorSpace="rgb",
               scale=32, G_clamp=5, G_L1=0, G_L2=0, N_epoch=10000, noiseDim=100)                    # pretrain_g.lua:12-29
    for k, v in lua.items():
        assert getattr(o, k) == v, k
    assert (o.epochs, o.synthetic, o.dataDir, o.augment) == (0, False, "dataset/out_aug_64x64", False)
    tv = importlib.import_module("train_v").parse([])
    for k in vars(tv):
        if k.startswith("aug"):
            assert getattr(o, k) == getattr(tv, k), k


def test_output_file_name():
    pg = importlib.import_module("pretrain_g")
    assert pg.pretrained_filename("logs", (3, 32, 32), 100) == os.path.join("logs", "g_pretrained_3x32x32_nd100.net")
    assert pg.pretrained_filename("/x", (1, 64, 64), 256) == "/x/g_pretrained_1x64x64_nd256.net"


def test_train_parse_accepts_G_pretrained_dir(cg, tmp_path):
    tr = importlib.import_module("train")
    assert tr.parse([]).G_pretrained_dir == "logs"                                                   # train.lua:20
    assert tr.parse(["--G_pretrained_dir", "/some/where"]).G_pretrained_dir == "/some/where"
    assert tr.load_pretrained_G(cg, str(tmp_path), (3, 32, 32), 100) is None                         # no file: the caller builds a fresh G


def test_t7_round_trip_of_decoder_and_autoencoder(cg, tmp_path):
    t7 = importlib.import_module("cat-generator_amd.t7")
    t7_nn = importlib.import_module("cat-generator_amd.t7_nn")
    cg.manual_seed(4)
    A = cg.models.create_G_autoencoder((3, 32, 32), 100)
    A.get(1).modules[1].running_mean.copy(np.linspace(-1, 1, 16).astype(np.float32))
    fn = str(tmp_path / "ae.net")
    t7.save(fn, {"G": t7_nn.to_t7(A.get(2)), "AE": t7_nn.to_t7(A), "EPOCH": 3})
    z = t7.load(fn)
    for src, key in ((A.get(2), "G"), (A, "AE")):
        back = t7_nn.from_t7(z[key])
        assert [m.typename for m in back.listModules()] == [m.typename for m in src.listModules()]
        np.testing.assert_array_equal(back.getParameters()[0].numpy(), src.getParameters()[0].numpy())
    back = t7_nn.from_t7(z["AE"])
    np.testing.assert_array_equal(back.get(1).modules[1].running_mean.numpy(), np.linspace(-1, 1, 16).astype(np.float32))
    assert z["EPOCH"] == 3
