"""vo_conv1d_plane_takes (include/vonoma.h): which vo_conv1d calls the MRF stage-0 plane conv (csrc/conv_plane.hip)
takes, checked without a GPU on descriptors with placeholder pointers (as tests/test_conv1d_plan.py), and that the
launch record of such a call stays the 256 x 256 stage-0 tile's."""

import ctypes

import pytest

import test_conv1d_plan as P
from visual_onoma_to_wave_amd import _lib

S0 = dict(P.S0)  # variant 1, res1 + res2, leaky-ReLU prologue, scale 1 / 3
RECORD = P._rec(256, 256, 4, 4, (2, 2, 2), _lib.VO_BF16, role=1)


def _takes(d):
    return _lib.lib().vo_conv1d_plane_takes(ctypes.byref(d))


def _s0(K=7, dil=3, C=256, **kw):
    return P._desc(5, 773, C, C, K, dil=dil, **{**S0, **kw})


@pytest.mark.parametrize("K", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_takes_the_stage0_convs(K, dil):
    d = _s0(K, dil)
    assert _takes(d) == 1
    assert P._plan(d) == (0, RECORD)
    c1 = _s0(K, dil, res1=False, res2=False, scale=1.0, post=_lib.ACT_LRELU, post_slope=0.1)
    assert _takes(c1) == 1 and P._plan(c1) == (0, RECORD)
    # c2 as Generator calls it: no prologue activation (c1's epilogue applied it)
    c2 = _s0(K, 1, pre=_lib.ACT_NONE, pre_slope=0.0)
    assert _takes(c2) == 1 and P._plan(c2) == (0, RECORD)


REFUSED = {
    "lens": dict(lens=True),
    "C128": dict(C=128),
    "K5": dict(K=5, dil=1),
    "f32-out": dict(ydt="f32"),
    "ldy264": dict(ldy=264),
    "no-bias": dict(bias=False),
    "workspace": None,  # built below: a scratch pointer on the stage-0 descriptor
    "halo66": dict(K=3, dil=33),
    "halo66-k7": dict(K=7, dil=11),
    "relu-prologue": dict(pre=_lib.ACT_RELU),
    "tanh-post": dict(post=_lib.ACT_TANH),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_leaves_the_rest_to_the_tiled_kernel(name):
    if name == "workspace":
        d = _s0()
        d.workspace, d.workspace_bytes = P.PTR, 1 << 20
    else:
        d = _s0(**REFUSED[name])
    assert _takes(d) == 0


def test_conv_cfg_selects_the_tiled_kernels():
    """conv_cfg 5 / 6 / 9 keep the call on the tiled kernels (the record is the same tile's); 0 again: the plane conv."""
    d = _s0()
    try:
        for cfg in (5, 6, 9):
            _lib.lib().vo_tune(b"conv_cfg", cfg)
            assert _takes(d) == 0 and P._plan(d) == (0, RECORD)
    finally:
        _lib.lib().vo_tune(b"conv_cfg", 0)
    assert _takes(d) == 1


def test_null_descriptor():
    assert _lib.lib().vo_conv1d_plane_takes(None) == 0
