"""--scale 16 without a GPU: the models create_G / create_D return at 16 px (models.lua:108-132 G16up, :640-711 D32_st3) against
the oracle's, and their plans in trace mode - the localisation branches of D's three branch transformers (4x4 maps of 64 planes behind
the pooling) as one cg_locnet_forward / _backward launch, so that D at 16 px costs no more launches than D at 32 px."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_trace as T  # noqa: E402
import scale16 as S16  # noqa: E402
from oracle import oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def cg():
    return S16.cg_pkg()


@pytest.mark.parametrize("ch,nG", [(3, 1849862), (1, 1847556)])
def test_models_at_16px_are_the_reference_ones(cg, ch, nG):
    G, Go = S16.pair(cg, 41, "G", ch)
    kinds = [type(m).__name__ for m in G.modules]
    assert kinds == ["Linear", "View", "PReLU",
                     "SpatialUpSamplingNearest", "SpatialConvolution", "SpatialBatchNormalization", "PReLU",
                     "SpatialUpSamplingNearest", "SpatialConvolution", "SpatialBatchNormalization", "PReLU",
                     "SpatialConvolution", "Sigmoid"]
    assert all(G.modules[i].typename == "cudnn.SpatialConvolution" for i in (4, 8, 11))
    assert tuple(G.modules[0].weight.shape) == (2048, 100) and tuple(G.modules[1].sizes) == (128, 4, 4)
    convs = [(m.nInputPlane, m.nOutputPlane, m.kW, m.padW) for m in G.modules if type(m).__name__ == "SpatialConvolution"]
    assert convs == [(128, 256, 5, 2), (256, 128, 5, 2), (128, ch, 3, 1)]
    pG, _ = G.getParameters(); pGo, _ = O.get_parameters(Go)
    assert pG.nElement() == nG
    np.testing.assert_array_equal(pG.numpy(), pGo)
    D, Do = S16.pair(cg, 42, "D", ch)
    pD, _ = D.getParameters(); pDo, _ = O.get_parameters(Do)
    if ch == 3:
        assert pD.nElement() == 2646601
    np.testing.assert_array_equal(pD.numpy(), pDo)
    # what create_G returns at 16 px is the 16 px decoder, and the 32 px decoder is unchanged by its `base` argument
    assert cg.models.create_G_decoder_upsampling16((ch, 16, 16), 100).modules[0].weight.shape[0] == 2048
    assert cg.models.create_G_decoder_upsampling32((ch, 32, 32), 100).modules[0].weight.shape[0] == 8192


def test_locnet_supported_lists_the_4x4_branch_shape_only(cg):
    L = cg.lib()
    for P in (1, 2, 3, 4):
        assert L.locnet_supported(4, 64, P) == 1
    for S, Cin, P in ((4, 3, 1), (4, 8, 4), (4, 16, 4), (4, 32, 4), (4, 128, 4), (2, 64, 4), (4, 64, 5), (4, 64, 0), (6, 64, 4)):
        assert L.locnet_supported(S, Cin, P) == 0, (S, Cin, P)
    for S, Cin, P in ((8, 64, 4), (16, 3, 1), (8, 3, 1), (8, 8, 4)):
        assert L.locnet_supported(S, Cin, P) == 1, (S, Cin, P)


@pytest.mark.parametrize("N", [8, 128])
def test_plan_of_the_discriminator_at_16px(N):
    r = S16.trace_D16(N)
    f, b = r["forward"], r["backward"]
    loc = T.calls(f, "cg_locnet_forward")
    assert [(a["ngroups"], a["x_shared"], a["S"], a["Cin"], a["P"]) for _, a in loc] == [("i:1", "i:1", "i:8", "i:3", "i:1"),
                                                                                       ("i:3", "i:1", "i:4", "i:64", "i:4")]
    assert [a["n_per_group"] for _, a in loc] == [f"i:{N}"] * 2
    names = [c[0] for c in T.calls(f)]
    assert not [n for n in names if n.startswith(("cg_affine_", "cg_avgpool2_", "cg_leakyrelu_"))]
    lb = T.calls(b, "cg_locnet_backward")
    assert [a["ngroups"] for _, a in lb] == ["i:3", "i:1"]
    assert [(a["S"], a["Cin"], a["P"]) for _, a in lb] == [("i:4", "i:64", "i:4"), ("i:8", "i:3", "i:1")]
    for i, l in enumerate(b):
        if "cg_locnet_backward" in l:      # each followed by the four deferred weight gradients of its layers, behind the fork
            assert b[i + 1].startswith("event|record|wgfork") and b[i + 2].startswith("event|wait|wgfork")
            assert all("cg_conv2d_wgrad_grouped_deferred" in x for x in b[i + 3:i + 7])
    # the yardstick: the same network at 32 px, traced here
    r32 = T.trace("D32_st3", N)
    assert r["stats"]["programs"] == 1
    assert r["stats"]["launches_forward"] <= r32["stats"]["launches_forward"]
    assert r["stats"]["launches_backward"] <= r32["stats"]["launches_backward"]
    assert len(T.calls(f)) <= len(T.calls(r32["forward"])) and len(T.calls(b)) <= len(T.calls(r32["backward"]))
    # fuse_locnet 2 (ungrouped localisation branches only): the first transformer's launch, the branch nets module by module
    r2 = S16.trace_D16(N, options=[("fuse_locnet", 2)])
    loc2 = T.calls(r2["forward"], "cg_locnet_forward")
    assert [(a["ngroups"], a["S"], a["Cin"]) for _, a in loc2] == [("i:1", "i:8", "i:3")]
    n2 = [c[0] for c in T.calls(r2["forward"])]
    assert "cg_affine_matrix_forward" in n2 and "cg_affine_grid_forward" in n2 and "cg_avgpool2_forward" in n2
    assert [a["ngroups"] for _, a in T.calls(r2["backward"], "cg_locnet_backward")] == ["i:1"]
    assert r2["stats"]["launches_forward"] > r["stats"]["launches_forward"] and r2["stats"]["launches_backward"] > r["stats"]["launches_backward"]


def test_plan_of_the_generator_at_16px():
    r = S16.trace_G16(128)
    f = [c[0] for c in T.calls(r["forward"])]
    assert r["stats"]["programs"] == 1 and r["stats"]["launches_forward"] == 11 and len(f) == 11
    # conv -> BN -> PReLU: statistics partials from the GEMM epilogue; the 256 -> 128 5x5 layer's phases in Winograd F(2x2,3x3)
    assert f.count("cg_bn_stats_finalize") == 2 and "cg_bn_stats" not in f and f.count("cg_bn_act_forward") == 2
    assert f.count("cg_conv2d_ups2_wino_forward_stats") == 1
    assert "cg_upsample2x_forward" not in f and f[-1] == "cg_sigmoid_forward"
    small = S16.trace_G16(8)
    assert small["stats"]["launches_forward"] == 11


def test_autoencoder_at_16px_still_refuses_and_says_why(cg):
    with pytest.raises(NotImplementedError, match="create_G_encoder16"):
        cg.models.create_G_autoencoder((3, 16, 16), 100)
