"""CPU self-test of the conv1d checker (tests/conv_check.py) and the static coverage check of the GPU tile
matrix (tests/test_gpu_conv1d_tiles.py).  The checker must accept a plain fp32 F.conv1d on the same
operands -- and that result rounded to bf16 under the bf16-output bar -- and reject each deliberate fault."""

import pytest

import conv_check as CC
from conv_check import ACT_LRELU, ACT_RELU, case

# shallow and deep reductions, ragged channels, a strided grouped conv, residual epilogue; every x has guard
# rows around each utterance and sentinel channels past Ci
SHAPES = [
    dict(a=(2, 65, 64, 128, 3)),
    dict(a=(2, 33, 1024, 64, 9)),                                     # R = 9216
    dict(a=(2, 65, 40, 20, 3), kw=dict(pre=ACT_LRELU)),
    dict(a=(2, 131, 64, 96, 5), kw=dict(stride=2, groups=2)),
    dict(a=(2, 65, 64, 128, 3), kw=dict(res1=True, res2=True, scale=0.5, post=ACT_RELU)),
]
MUTATIONS = ["drop_tap", "drop_channel", "shift_row", "zero_group", "guard", "leak_channel"]


def _case(sh, ydt):
    return case(*sh["a"], cdt="bf16", xdt="bf16", ydt=ydt, x_rows=2, ldx_extra=8, ldy_extra=0 if sh.get("kw", {}).get(
        "res1") else 4, **sh.get("kw", {}))


def _check(c, mutate=None):
    m = CC.make(c)
    ref, bar = CC.reference(c, m)
    CC.torch_conv(c, m, mutate)
    return CC.verify(c, m, ref, bar)


@pytest.mark.parametrize("ydt", ["f32", "bf16"])
@pytest.mark.parametrize("sh", SHAPES, ids=[str(s["a"]) for s in SHAPES])
def test_checker_accepts_fp32_conv(sh, ydt):
    ratio, rel = _check(_case(sh, ydt))
    assert ratio <= 1.0
    if ydt == "f32":  # the element bar is a worst-case bound: a correct fp32 conv sits far below it
        assert ratio < 0.05 and rel < 1e-6


@pytest.mark.parametrize("ydt", ["f32", "bf16"])
@pytest.mark.parametrize("mutate", MUTATIONS)
@pytest.mark.parametrize("sh", SHAPES[:2], ids=[str(s["a"]) for s in SHAPES[:2]])
def test_checker_rejects_mutation(sh, mutate, ydt):
    c = _case(sh, ydt)
    with pytest.raises(AssertionError):
        _check(c, mutate)


def test_drop_tap_fails_most_elements():
    """The element bar alone (not the whole-tensor one) rejects a dropped tap on most elements."""
    c = _case(SHAPES[0], "f32")
    m = CC.make(c)
    ref, bar = CC.reference(c, m)
    CC.torch_conv(c, m, "drop_tap")
    over = ((m["y"].double() - ref).abs() > bar).double().mean()
    assert float(over) > 0.8, float(over)


def test_tile_matrix_covers_required_instantiations():
    """Every conv1d_kernel instantiation the dispatcher can reach with default knobs (REQUIRED, written by
    hand from select_types / select_disc) is declared by a case of the GPU matrix, which asserts it at run
    time through the launch record."""
    import test_gpu_conv1d_tiles as M
    declared = {CC.instantiation(c) for c in M.CASES}
    missing = sorted(set(M.REQUIRED) - declared)
    assert not missing, missing
    assert len(set(M.REQUIRED)) >= 100
    for c in M.CASES:  # T one past a tile multiple (or a single short tile), bf16-output cases have an fp32 twin
        bt = c["tile"][1]
        assert c["tile"][3] == 1 or c["T_out"] <= bt or c["T_out"] % bt in (1, 5), c["name"]
        if c["ydt"] == "bf16":
            twin = dict(c, ydt="f32")
            assert any(all(o[k] == twin[k] for k in twin if k not in ("name", "seed")) for o in M.CASES), c["name"]


def test_rejected_conv1d_leaves_a_zero_launch_record():
    """Host side of vo_conv1d_last_launch (no kernel is launched: every call here is refused by the argument
    checks): a rejected call reads as zeros, VO_F32X3 with transposed is rejected before the upsampler
    dispatch, and the copy is clamped to n."""
    import ctypes
    import torch
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    d = _lib.Conv1dDesc()
    d.x = d.w = d.y = 4096  # never dereferenced: the call is refused on the host
    d.x_dtype = d.y_dtype = _lib.VO_F32
    d.B, d.T_in, d.T_out, d.Ci, d.Co, d.K, d.dil, d.pad = 2, 16, 17, 128, 128, 2, 1, 1
    d.ldx, d.ldy, d.x_bstride, d.y_bstride = 128, 64, 16 * 128, 32 * 64
    d.out_scale, d.compute_dtype = 1.0, _lib.VO_F32X3
    d.transposed, d.up_stride, d.up_pad, d.up_cout, d.up_tout = 1, 2, 1, 64, 32
    assert L.vo_conv1d(ctypes.byref(d), None) == -1
    assert b"F32X3" in L.vo_last_error() and b"transposed" in L.vo_last_error()
    assert set(ops.conv1d_last_launch().values()) == {0}
    assert len(ops.LAUNCH_FIELDS) == 13
    rec = (ctypes.c_int32 * 16)(*([7] * 16))
    assert L.vo_conv1d_last_launch(rec, 3) == 3 and list(rec[:4]) == [0, 0, 0, 7]
    assert L.vo_conv1d_last_launch(rec, 64) == 13 and L.vo_conv1d_last_launch(None, 13) == 0
    with pytest.raises(ValueError, match="F32X3"):  # the Python guard fires before any device work
        ops.conv1d(torch.zeros(2, 16, 128), torch.zeros(2, 128, 128), None, Co=128, K=2, pad=1,
                   transposed=dict(stride=2, pad=1, cout=64), compute_dtype=ops.F32X3)
