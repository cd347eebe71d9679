"""vo_conv1d_plan (include/vonoma.h): the tile rule of vo_conv1d checked without a GPU.  The plan runs the
dispatcher's argument checks and selection on the host alone and reports the launch record vo_conv1d would leave.
Expected records are the hand-written tables of tests/test_gpu_conv1d_tiles.py (CASES: proved on an MI355X through
vo_conv1d_last_launch) and, for the forms that matrix leaves out, records written by hand from the dispatcher's
rules -- never read back from the code under test.  Descriptors carry placeholder pointers: no tensor is read."""

import ctypes
import functools

import pytest

import conv_check as CC
import test_gpu_conv1d_tiles as M
from visual_onoma_to_wave_amd import _lib, ops

PTR = 4096  # any non-null value: vo_conv1d_plan dereferences no tensor pointer
VO = {"f32": _lib.VO_F32, "bf16": _lib.VO_BF16}


def _plan(d):
    """(rc, record dict) of vo_conv1d_plan."""
    rec = (ctypes.c_int32 * len(ops.LAUNCH_FIELDS))(*([7] * len(ops.LAUNCH_FIELDS)))
    rc = _lib.lib().vo_conv1d_plan(ctypes.byref(d), rec, len(ops.LAUNCH_FIELDS))
    return rc, dict(zip(ops.LAUNCH_FIELDS, (int(v) for v in rec)))


def _rec(bco, bt, ni, wco, sizes, cdt, s=1, seg=0, nice=1, splits=1, role=0):
    return dict(BCO=bco, BT=bt, S=s, SEG=seg, nice=nice, splits=splits, sizeof_in=sizes[0], sizeof_compute=sizes[1],
                sizeof_out=sizes[2], ROLE=role, compute_dtype=cdt, NI=ni, WCO=wco)


def _desc(B, T, Ci, Co, K, *, xdt="bf16", cdt=_lib.VO_BF16, ydt="bf16", dil=1, pad=None, T_out=None, ldx=None, ldy=None,
          x_rows=None, y_rows=None, stride=1, groups=1, bias=True, res1=False, res2=False, pre=0, pre_slope=0.0, post=0,
          post_slope=0.0, scale=1.0, variant=0, lens=False, up=None, workspace=False):
    """A vo_conv1d_desc as ops.conv1d builds it from tensors of these shapes (up = (stride, pad, cout): the polyphase
    ConvTranspose1d).  workspace: ask vo_conv1d_workspace_size and set a scratch of that size, as ops.conv1d does."""
    d = _lib.Conv1dDesc()
    pad = dil * (K - 1) // 2 if pad is None else pad
    d.x = d.w = d.y = PTR
    d.x_dtype, d.y_dtype, d.compute_dtype = VO[xdt], VO[ydt], cdt
    d.bias = PTR if bias else None
    d.res1, d.res2 = (PTR if res1 else None), (PTR if res2 else None)
    d.B, d.T_in, d.Ci, d.Co, d.K, d.dil, d.pad = B, T, Ci, Co, K, dil, pad
    d.ldx = ldx or Ci
    d.x_bstride = (x_rows or T) * d.ldx
    if up is not None:
        s, p, cout = up
        d.transposed, d.up_stride, d.up_pad, d.up_cout, d.up_tout = 1, s, p, cout, T * s + s - 2 * p
        d.T_out, d.ldy, d.y_bstride = T + 1, cout, d.up_tout * cout
    else:
        d.T_out = T_out if T_out is not None else (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
        d.ldy = ldy or Co
        d.y_bstride = (y_rows or d.T_out) * d.ldy
    d.pre_act, d.pre_slope, d.post_act, d.post_slope, d.out_scale = pre, pre_slope, post, post_slope, scale
    d.variant, d.stride, d.groups = variant, stride, groups
    if lens:
        d.lens, d.lens_scale = PTR, 1
    if workspace:
        nb = _lib.lib().vo_conv1d_workspace_size(ctypes.byref(d))
        assert nb > 0
        d.workspace, d.workspace_bytes = PTR, nb
    return d


def _case_desc(c):
    """The descriptor ops.conv1d builds for a case of the GPU tile matrix (the views of conv_check.make)."""
    strided = not (c["res1"] or c["res2"])
    d = _desc(c["B"], c["T"], c["Ci"], c["Co"], c["K"], xdt=c["xdt"], cdt=VO[c["cdt"]], ydt=c["ydt"], dil=c["dil"],
              pad=c["pad"], T_out=c["T_out"], ldx=c["Ci"] + c["ldx_extra"], x_rows=c["T"] + 2 * c["x_rows"],
              ldy=c["Co"] + (c["ldy_extra"] if strided else 0), y_rows=c["T_out"] + (c["y_rows"] if strided else 0),
              stride=c["stride"], groups=c["groups"], bias=c["bias"], res1=c["res1"], res2=c["res2"], pre=c["pre"],
              pre_slope=c["pre_slope"], post=c["post"], post_slope=c["post_slope"], scale=c["scale"])
    if c["stride"] <= 1 and c["groups"] <= 1 and c["cdt"] == "f32" and c["T_out"] <= 16:
        # ops.conv1d's workspace pre-filter (the short fp32 convs): a scratch where the library wants one
        nb = _lib.lib().vo_conv1d_workspace_size(ctypes.byref(d))
        if nb > 0:
            d.workspace, d.workspace_bytes = PTR, nb
    return d


@pytest.mark.parametrize("c", M.CASES, ids=[c["name"] for c in M.CASES])
def test_plan_matches_the_tile_matrix(c):
    rc, rec = _plan(_case_desc(c))
    assert rc == 0, _lib.lib().vo_last_error()
    assert rec == CC.record(c), (c["name"], rec, CC.record(c))


F, BF, X3 = _lib.VO_F32, _lib.VO_BF16, _lib.VO_F32X3
S0 = dict(variant=1, res1=True, res2=True, pre=_lib.ACT_LRELU, pre_slope=0.1, scale=1.0 / 3)
UPS0 = dict(up=(8, 4, 256), pre=_lib.ACT_LRELU, pre_slope=0.1)
NAMES = ("splitk-f32-w1", "splitk-f32-w2", "splitk-f32x3-w1", "splitk-bf16-deep", "bf16-deep-no-workspace", "stage0-k3",
         "stage0-k7", "stage0-k3-lens", "stage0-k7-lens", "conv-pre-lens", "ups0-small-lens", "ups0", "ups-128",
         "ups-64-lens", "ups-wide")
ZERO = dict.fromkeys(ops.LAUNCH_FIELDS, 0)


@functools.lru_cache(maxsize=None)
def _extra():
    """name -> (descriptor, record written by hand from the dispatcher's rules: csrc/conv1d.hip select_types,
    select_role, splitk_plan).  Built on first use: the workspace query loads the library."""
    e = _extra_tiled()
    # polyphase upsamplers the streaming kernel (upsample.hip) takes: no conv1d_kernel tile, an all-zero record
    for name, ci, up, lens in (("ups-128", 128, (2, 1, 64), False), ("ups-64-lens", 64, (2, 1, 32), True),
                               ("ups-wide", 256, (8, 4, 128), False)):
        e[name] = (_desc(2, 40, ci, up[0] * up[2], 2, pad=1, bias=False, up=up, lens=lens), ZERO)
    assert set(e) == set(NAMES)
    return e


def _extra_tiled():
    return {
    # tests/test_gpu_splitk.py, fp32 at T_out <= 16 with a workspace: FFN w_1 (8 chunks x 9 taps: one chunk per split)
    # on the 64-channel SEG tile, FFN w_2 (32 chunks, 4 per split) on the 32-channel one; the same in split-bf16
    "splitk-f32-w1": (_desc(32, 12, 256, 1024, 9, xdt="f32", cdt=F, ydt="f32", post=_lib.ACT_RELU, scale=0.5,
                            workspace=True), _rec(64, 64, 2, 2, (4, 4, 4), F, seg=1, splits=8)),
    "splitk-f32-w2": (_desc(32, 12, 1024, 256, 1, xdt="f32", cdt=F, ydt="f32", res1=True, scale=0.5, workspace=True),
                      _rec(32, 64, 1, 2, (4, 4, 4), F, seg=1, splits=8)),
    "splitk-f32x3-w1": (_desc(32, 12, 256, 1024, 9, xdt="f32", cdt=X3, ydt="f32", post=_lib.ACT_RELU, workspace=True),
                        _rec(64, 64, 2, 2, (4, 4, 4), X3, seg=1, splits=8)),
    # the deep bf16 form (FFN w_1 input gradient, 1024 -> 256 k9 at 8192 rows: 32 chunks, 32 256 x 256 tiles -> 8 splits
    # of 4 chunks) on the 256 x 256 tile; without a workspace the Co <= 256 rule's 64 x 128 tile
    "splitk-bf16-deep": (_desc(16, 512, 1024, 256, 9, bias=False, workspace=True),
                         _rec(256, 256, 4, 4, (2, 2, 2), BF, splits=8)),
    "bf16-deep-no-workspace": (_desc(16, 512, 1024, 256, 9, bias=False), _rec(64, 128, 2, 2, (2, 2, 2), BF)),
    # MRF stage 0 (variant 1, C = 256): its own ROLE on the 256 x 256 tile, k = 3 (weights by DMA) and k = 7 (role split)
    "stage0-k3": (_desc(5, 773, 256, 256, 3, **S0), _rec(256, 256, 4, 4, (2, 2, 2), BF, role=1)),
    "stage0-k7": (_desc(5, 773, 256, 256, 7, **S0), _rec(256, 256, 4, 4, (2, 2, 2), BF, role=1)),
    "stage0-k3-lens": (_desc(5, 773, 256, 256, 3, lens=True, **S0), _rec(256, 256, 4, 4, (2, 2, 2), BF, role=1)),
    "stage0-k7-lens": (_desc(5, 773, 256, 256, 7, dil=5, lens=True, **S0), _rec(256, 256, 4, 4, (2, 2, 2), BF, role=1)),
    # ragged conv_pre reading an fp32 mel (80 -> 512 k7, 985 rows <= 2048: 64 x 64; Ci = 80 is no multiple of 32)
    "conv-pre-lens": (_desc(5, 197, 80, 512, 7, xdt="f32", lens=True), _rec(64, 64, 2, 2, (4, 2, 2), BF, nice=0)),
    # ups0 (512 -> 8 x 256 phase columns) stays on the tiled conv: 64 x 64 at 990 rows, 256 x 256 at the vocoder's size
    "ups0-small-lens": (_desc(5, 197, 512, 2048, 2, pad=1, lens=True, **UPS0), _rec(64, 64, 2, 2, (2, 2, 2), BF)),
    "ups0": (_desc(32, 512, 512, 2048, 2, pad=1, **UPS0), _rec(256, 256, 4, 4, (2, 2, 2), BF)),
    }


@pytest.mark.parametrize("name", NAMES)
def test_plan_of_the_forms_outside_the_matrix(name):
    d, want = _extra()[name]
    rc, rec = _plan(d)
    assert rc == 0, _lib.lib().vo_last_error()
    assert rec == want, (name, rec, want)


def test_refusals_match_vo_conv1d():
    """A refused descriptor returns -1 from vo_conv1d and vo_conv1d_plan with the same vo_last_error, and a zero
    record (both are refused on the host, before any launch)."""
    L = _lib.lib()
    x3 = _desc(2, 16, 128, 128, 2, xdt="f32", cdt=X3, ydt="f32", pad=1, bias=False, up=(2, 1, 64))
    strided = _desc(2, 64, 64, 64, 3, stride=2, lens=True)
    for d, word in ((x3, b"VO_F32X3 compute excludes transposed"), (strided, b"lens excludes stride")):
        assert L.vo_conv1d(ctypes.byref(d), None) == -1
        err = L.vo_last_error()
        assert word in err
        rc, rec = _plan(d)
        assert rc == -1 and L.vo_last_error() == err and rec == ZERO


def test_plan_leaves_the_last_launch_record_alone():
    """The calling thread's record reads the same before and after a plan, accepted or refused, and the copy is
    clamped to n like vo_conv1d_last_launch's."""
    L = _lib.lib()
    before = ops.conv1d_last_launch()
    d, want = _extra()["stage0-k7"]
    assert _plan(d) == (0, want) and ops.conv1d_last_launch() == before
    assert _plan(_desc(2, 64, 64, 64, 3, stride=2, lens=True))[0] == -1 and ops.conv1d_last_launch() == before
    rec = (ctypes.c_int32 * 16)(*([7] * 16))
    assert L.vo_conv1d_plan(ctypes.byref(d), rec, 3) == 0 and list(rec[:4]) == [256, 256, 1, 7]
    assert L.vo_conv1d_plan(ctypes.byref(d), rec, 64) == 0 and list(rec[9:14]) == [1, BF, 4, 4, 7]
    assert L.vo_conv1d_plan(ctypes.byref(d), None, 13) == 0
