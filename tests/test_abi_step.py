"""The drop-in boundary without its Python host: one whole D+G update (adversarial.lua:51-275) recorded as a sequence of
C-ABI calls and replayed by tools/abi_replay - a plain C++ program that owns its device memory (cg_malloc), its stream
(cg_stream_create) and dispatches every call by name through a table generated from include/catgan.h.  No interpreter,
no PyTorch in that process.

Two recordings:
  * the PLANNED step at the benchmarked batch (128): the description of G32up-c and D32_st3 (cg_net_create / _add / _bind), then one
    cg_net_forward / cg_net_backward per pass - the two generator forwards as one cg_net_forward_pair - with the batch assembly,
    criterion and optimiser calls between them: the path AND the schedule bench.py times, as a LuaJIT host issues it (lua/catgan/net.lua);
  * the per-module walk at a small batch: one C call per nn.Module method, the sequence the per-module classes of
    lua/catgan/nn.lua issue (the LuaJIT layer cannot run in this image; scripts/check_lua_binding.py checks its C calls against
    the header statically).
Either replay must reproduce the Python host's parameter vectors exactly."""
import importlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
f32 = np.float32

_CHILD = r"""
import importlib, os, sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tools"))
from abi_record import Recorder
cg = importlib.import_module("cat-generator_amd")
cg.nn.planned = {planned}
N = {N}
cg.manual_seed(91)
G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
S = cg.adversarial.State(dict(batchSize=N), G, D)
S.device_rng = True      # real-batch indices from the device generator: nothing but ABI calls touches the device
data = cg.adversarial.TrainData(np.random.RandomState(4).rand(2 * N, 3, 32, 32).astype(np.float32))
cg.adversarial.iteration(S, data, N)      # warm-up: every buffer exists, weights are packed, plans are compiled
torch.cuda.synchronize()
rec = Recorder(cg)
rec.start()
cg.adversarial.iteration(S, data, N)      # the recorded update
torch.cuda.synchronize()
pD, pG = S.PARAMETERS_D, S.PARAMETERS_G
out = {out!r}
ncalls = rec.stop({{os.path.join(out, "pD.bin"): (pD.ptr, pD.nElement() * 4), os.path.join(out, "pG.bin"): (pG.ptr, pG.nElement() * 4)}},
                  os.path.join(out, "step.trace"), os.path.join(out, "step.blob"))
pD.numpy().tofile(os.path.join(out, "pD.ref")); pG.numpy().tofile(os.path.join(out, "pG.ref"))
print("NCALLS", ncalls)
"""


def _record_and_replay(tmp_path, planned, N):
    """Record in a fresh process (its device memory image is the blob: nothing of this test session is in it), replay, compare."""
    exe = os.path.join(ROOT, "tools", "abi_replay")
    assert os.path.exists(exe), "tools/abi_replay is built by __graft_entry__.build()"
    env = dict(os.environ, CG_NET_ALLOC="lib")     # plan buffers from the library's own allocator, as in a LuaJIT host
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, planned=planned, N=N, out=str(tmp_path))], capture_output=True,
                       text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ncalls = int(r.stdout.split("NCALLS")[1].split()[0])
    trace, blob = str(tmp_path / "step.trace"), str(tmp_path / "step.blob")
    names = [l.split("|")[1] for l in open(trace) if l.startswith("call|")]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "cat-generator_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, trace, blob], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{ncalls} calls replayed" in r.stdout, r.stdout
    out = {}
    for k in ("pD", "pG"):
        out[k] = (np.fromfile(str(tmp_path / f"{k}.bin"), dtype=f32), np.fromfile(str(tmp_path / f"{k}.ref"), dtype=f32))
    return names, out


@pytest.mark.gpu
def test_planned_step_at_the_benchmarked_batch_replayed_without_python(tmp_path):
    names, out = _record_and_replay(tmp_path, True, 128)
    assert names.count("cg_net_create") == 2 and names.count("cg_net_add") > 120            # G32up-c (17 modules) + D32_st3
    # G: fake generation (N/2) + the G-step's forward (N) as ONE cg_net_forward_pair + its join - the BENCHMARKED schedule, issued below the ABI
    # (round 6; round 5's host-side streams and events were invisible to this recording); D: the D-step's and the G-step's forward
    assert names.count("cg_net_forward_pair") == 1 and names.count("cg_net_pair_join") == 1 and names.count("cg_net_forward") == 2
    assert names.index("cg_net_forward_pair") < names.index("cg_net_forward") < names.index("cg_net_pair_join")
    assert names.count("cg_net_backward") == 3        # D backward, D updateGradInput, G backward
    per_module = [n for n in names if n.startswith(("cg_conv2d", "cg_prelu", "cg_bn_", "cg_act_pool", "cg_bilinear", "cg_affine", "cg_avgpool",
                                                    "cg_maxpool", "cg_mask_mul", "cg_sigmoid", "cg_leakyrelu", "cg_pack_"))]
    assert not per_module, f"the planned step issues no per-module launch through the host: {per_module[:5]}"
    for must in ("cg_gather_rows", "cg_rng_uniform_dev", "cg_bce_forward", "cg_bce_backward", "cg_adam_step", "cg_confusion_update"):
        assert must in names, f"{must} missing from the recorded step"
    assert len(names) < 400                                                                   # builders included
    np.testing.assert_array_equal(out["pD"][0], out["pD"][1])
    np.testing.assert_array_equal(out["pG"][0], out["pG"][1])


@pytest.mark.gpu
def test_per_module_step_replayed_without_python(tmp_path):
    names, out = _record_and_replay(tmp_path, False, 8)
    assert len(names) > 300 and not any(n.startswith("cg_net_") for n in names)
    for must in ("cg_conv2d_forward", "cg_conv2d_wgrad", "cg_conv2d_dgrad_ups2", "cg_prelu_backward", "cg_bn_forward", "cg_bn_backward",
                 "cg_bilinear_sampler_backward", "cg_adam_step", "cg_pack_conv_weight", "cg_rng_bernoulli_dev", "cg_bce_backward"):
        assert must in names, f"{must} missing from the recorded step"
    assert not any("grouped" in n or n in ("cg_conv2d_forward_ex", "cg_act_pool2_mask_forward", "cg_bn_act_forward") for n in names), \
        "the recorded host must be the plain one-call-per-module layer"
    np.testing.assert_array_equal(out["pD"][0], out["pD"][1])
    np.testing.assert_array_equal(out["pG"][0], out["pG"][1])


def test_lua_binding_calls_match_the_header():
    """scripts/check_lua_binding.py: every C.cg_* call in lua/ names a declared entry point with the right arity, the block
    structure of every file balances, and every class models.lua / adversarial.lua instantiate is defined."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_lua_binding.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 problems" in r.stdout


def test_reference_host_files_resolve_against_the_lua_providers():
    """The `drop in unchanged` claim, as far as it can be held without a Lua interpreter: every `require`, every namespace call
    (torch.* nn.* cudnn.* image.* paths.* sys.* xlua.* optim.* cutorch.* DISP.*) and every method name that the reference's
    adversarial.lua / models.lua / train.lua / weight-init.lua / utils/nn_utils.lua / dataset.lua use has a provider under lua/ (or
    is standard Lua, or is defined by those files themselves).  The names come from the committed list
    tests/golden/lua_reference_names.json, or from a checkout of the reference named by CATGAN_REFERENCE, which must then agree with that
    list.  The checker is not vacuous: a name nobody provides is reported."""
    spec = importlib.util.spec_from_file_location("check_lua_binding", os.path.join(ROOT, "scripts", "check_lua_binding.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    errs, names = chk.check_reference(os.environ.get("CATGAN_REFERENCE"))
    assert errs == [], errs[:10]
    assert {"pl", "image", "paths", "display", "torch", "nn", "optim", "cutorch"} <= set(names["requires"])
    assert {"torch.load", "torch.save", "xlua.progress", "sys.clock", "image.save", "paths.concat", "nn.BatchNormalization"} <= set(names["calls"])
    assert "clearState" in names["methods"]
    # negative control: the same resolution over a list with three names nobody provides
    import copy
    import json
    import tempfile
    bad = copy.deepcopy(names)
    bad["requires"]["qt"] = ["train.lua:0"]
    bad["calls"]["torch.bogusFunction"] = ["train.lua:0"]
    bad["methods"]["bogusMethod"] = ["train.lua:0"]
    with tempfile.TemporaryDirectory() as td:
        chk.MANIFEST = os.path.join(td, "names.json")
        json.dump(bad, open(chk.MANIFEST, "w"))
        errs2, _ = chk.check_reference(os.path.join(td, "no-such-tree"))
    assert len(errs2) == 3 and any("qt" in e for e in errs2) and any("bogusFunction" in e for e in errs2) and any("bogusMethod" in e for e in errs2)


def test_replayer_dispatch_covers_every_compute_entry_point():
    """tools/abi_dispatch.inc (generated from the header) has an entry for every int-returning entry point whose arguments
    are device pointers and scalars - i.e. everything a training step can call."""
    cg = importlib.import_module("cat-generator_amd")
    protos = cg._abi.parse_header()
    inc = open(os.path.join(ROOT, "tools", "abi_dispatch.inc")).read()
    host_only = {"cg_comm_available", "cg_comm_init", "cg_comm_size", "cg_comm_version", "cg_device_count", "cg_get_option", "cg_malloc", "cg_set_option",
                 "cg_stream_create", "cg_stream_on_queue", "cg_abi_version", "cg_pack_conv_weight_batch", "cg_concat_channels",
                 "cg_split_channels", "cg_concat_channels_dropout", "cg_split_channels_masked",   # the last five: host int arrays (fused hosts only)
                 "cg_conv2d_wgrad_pending", "cg_host_alloc", "cg_event_create",
                 # the planned executor's host-only services: callbacks, tracing, introspection
                 "cg_net_set_allocator", "cg_net_set_hook", "cg_net_trace_region", "cg_net_trace_take", "cg_net_module_state", "cg_net_stats"}
    for name, (ret, _) in protos.items():
        if ret == "int" and name not in host_only:
            assert f'"{name}"' in inc, f"{name} has no dispatch entry (re-run scripts/gen_abi_dispatch.py)"
