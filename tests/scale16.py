"""What the 16 px tests share (a plain module, imported as tests/plan_trace.py is): the oracle's form of G16up, the engine / oracle
pairs of the two networks at 16 px, and a trace-mode pass over any module tree (tests/plan_trace.py builds only its named nets)."""
import importlib

import numpy as np
import torch

from oracle import oracle as O


def cg_pkg():
    return importlib.import_module("cat-generator_amd")


def oracle_G16up(channels, noise_dim, rng):
    """models.lua:108-132 create_G_decoder_upsampling16 from the oracle's modules: O.create_G32up with a 4x4 first map."""
    cd = "cudnn.SpatialConvolution"
    m = O.Sequential(
        O.Linear(noise_dim, 128 * 4 * 4, rng), O.View(128, 4, 4), O.PReLU(),
        O.UpSample2(), O.Conv(128, 256, 5, 2, rng, cd), O.SBN(256, rng), O.PReLU(),
        O.UpSample2(), O.Conv(256, 128, 5, 2, rng, cd), O.SBN(128, rng), O.PReLU(),
        O.Conv(128, channels, 3, 1, rng, cd), O.Sigmoid())
    return O.weight_init_heuristic(m, rng)


def pair(cg, seed, which, ch=3):
    """(engine net, oracle net) at 16 px from the same seed."""
    cg.manual_seed(seed); rng = O.RNG(seed)
    if which == "G":
        return cg.models.create_G((ch, 16, 16), 100), oracle_G16up(ch, 100, rng)
    return cg.models.create_D((ch, 16, 16)), O.create_D32_st3(ch, 16, rng)


def trace_net(net, ishape, fmt, N, options=()):
    """One forward + backward of `net` on a zero batch of N in trace mode (no GPU) -> dict(forward, backward: [lines], stats)."""
    cg = cg_pkg()
    P = importlib.import_module("cat-generator_amd.planned")
    net.getParameters()
    x = cg.Tensor(torch.zeros(N * int(np.prod(ishape))), (N,) + tuple(ishape), fmt)
    pn = P.PlannedNet(net, trace=True)
    L = cg.lib()
    for k, v in options:
        L.net_set_option(pn.h, k.encode(), int(v))
    L.net_trace_region(pn.h, x.ptr, x.t.numel() * 4)
    pn.forward(x)
    pn.take_trace()                       # first pass: weight packing included
    y = pn.forward(x)
    res = dict(forward=pn.take_trace().strip().split("\n"))
    gy = cg.Tensor(torch.zeros(int(np.prod(y.shape))), y.shape, y.fmt)
    L.net_trace_region(pn.h, gy.ptr, max(gy.t.numel() * 4, 4))
    pn.backward(x, gy, True)
    res["backward"] = pn.take_trace().strip().split("\n")
    res["stats"] = pn.stats()
    res["net"] = pn
    return res


def trace_D16(N, options=()):
    cg = cg_pkg()
    cg.manual_seed(3)
    return trace_net(cg.models.create_D((3, 16, 16)), (3, 16, 16), "nhwc", N, options)


def trace_G16(N, options=()):
    cg = cg_pkg()
    cg.manual_seed(3)
    return trace_net(cg.models.create_G((3, 16, 16), 100), (100,), "plain", N, options)
