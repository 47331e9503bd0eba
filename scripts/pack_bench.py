#!/usr/bin/env python
"""The weight re-packing after a parameter update, alone: cg_pack_conv_weight_ups2 without and with its Winograd filter pack for G32up's
three upsample -> conv layers, and cg_pack_conv_weight_batch for the plain layers of D32_st3 and of G32up-c, under CG_PACK_WIDE = 0 and 1 in turn in one process.
HIP events around `iters` back-to-back calls after 5, beside a device-to-device copy of the bytes the call reads and writes.
    python scripts/pack_bench.py [iters] [rounds]"""
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cg = importlib.import_module("cat-generator_amd")
a = [int(v) for v in sys.argv[1:]]
iters, rounds = (a + [50, 3][len(a):])[:2]
L, st = cg.lib(), cg.tensor.stream()
E = lambda n: torch.empty(int(n), dtype=torch.float32, device="cuda")
R = lambda *shape: torch.randn(*shape, dtype=torch.float32, device="cuda")


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def copy_of(nbytes):
    """a device-to-device copy that moves nbytes in all (half read, half written) on the same stream"""
    n = int(nbytes) // 8
    src, dst = E(n), E(n)
    return lambda: L.memcpy_d2d(st, dst.data_ptr(), src.data_ptr(), n * 4)


cases = []
for Cout, Cin, k in ((512, 512, 3), (256, 512, 3), (128, 256, 5)):
    w = R(Cout, Cin, k, k)
    n = L.pack_conv_weight_ups2_floats(Cout, Cin, k, (k - 1) // 2)
    wf, wb = E(n), E(n)
    nu = L.conv2d_ups2_wino_u_floats(Cin, Cout) if k == 5 else L.conv2d_ups2_wino22_u_floats(Cin, Cout)
    uf, ub = E(nu), E(nu)
    wpack = L.conv2d_ups2_wino_pack if k == 5 else L.conv2d_ups2_wino22_pack

    def ups(w=w, wf=wf, wb=wb, Cout=Cout, Cin=Cin, k=k):
        L.pack_conv_weight_ups2(st, w.data_ptr(), wf.data_ptr(), wb.data_ptr(), Cout, Cin, k, (k - 1) // 2)

    def both(ups=ups, wpack=wpack, wf=wf, wb=wb, uf=uf, ub=ub, Cout=Cout, Cin=Cin):
        ups()
        wpack(st, wf.data_ptr(), wb.data_ptr(), uf.data_ptr(), ub.data_ptr(), Cout, Cin)

    cases.append((f"ups2 pack {Cin}->{Cout} {k}x{k}", ups, 4 * (w.numel() + 2 * n)))
    cases.append((f"ups2 + {'F(2x2,3x3)' if k == 5 else 'F(2x2,2x2)'} pack {Cin}->{Cout} {k}x{k}", both, 4 * (w.numel() + 2 * n + 2 * n + 2 * nu)))

# the plain layers of a net as the planned pass packs them: D32_st3's View -> Linear(20480, 256) in the map layout (320 planes on the
# 8 x 8 map); G32up-c's layers that do not sit behind an upsampling (the noise's Linear(100, 32768) and the last convolution)
def batch_case(name, net):
    layers, prev = [], None
    for m in net.listModules():
        if m.typename in ("nn.SpatialConvolution", "cudnn.SpatialConvolution") and prev != "nn.SpatialUpSamplingNearest":
            co, ci, kh, kw = m.weight.shape
            layers.append((co, ci, kh, kw, 0))
        elif m.typename == "nn.Linear":
            co, ci = m.weight.shape
            layers.append((co, 320, 8, 8, 1) if ci == 20480 else (co, ci, 1, 1, 0))
        if m.typename != "nn.Sequential":
            prev = m.typename
    nl = len(layers)
    ws = [R(co, ci * kh * kw) for co, ci, kh, kw, _ in layers]
    sizes = [L.pack_conv_weight_floats(co, ci, kh, kw) for co, ci, kh, kw, _ in layers]
    wfs, wbs = [E(s) for s in sizes], [E(s) for s in sizes]
    ptrs = lambda ts: ctypes.cast((ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts]), ctypes.c_void_p)
    ints = lambda col: (ctypes.c_int * nl)(*[lay[col] for lay in layers])
    keep = (ws, wfs, wbs, ptrs(ws), ptrs(wfs), ptrs(wbs), ints(0), ints(1), ints(2), ints(3), ints(4))
    cases.append((f"batch pack, {name}'s {nl} plain layers", lambda k=keep: L.pack_conv_weight_batch(st, nl, *k[3:]),
                  4 * (sum(w.numel() for w in ws) + 2 * sum(sizes))))


batch_case("D32_st3", cg.models.create_D((3, 32, 32)))
batch_case("G32up-c", cg.models.create_G((3, 32, 32), 100))

out = []
for name, fn, nbytes in cases:
    cp = copy_of(nbytes)
    row = {"case": name, "bytes": nbytes, "us": {"0": [], "1": [], "copy": []}}
    for _ in range(rounds):
        for mode in (0, 1):
            L.set_option(b"CG_PACK_WIDE", mode)
            row["us"][str(mode)].append(round(timed(fn), 2))
        row["us"]["copy"].append(round(timed(cp), 2))
    L.set_option(b"CG_PACK_WIDE", -1)
    out.append(row)
    f = lambda v: "/".join(f"{x:.1f}" for x in v)
    print(f"{name:44s} {nbytes / 1e6:7.1f} MB   CG_PACK_WIDE=0 {f(row['us']['0'])} us   =1 {f(row['us']['1'])} us   copy {f(row['us']['copy'])} us")
print(json.dumps({"pack_bench": out, "iters": iters}))
