"""The MRF stage-0 plane conv (csrc/conv_plane.hip: vo_conv1d's dense variant-1 calls at C = 256, k = 3 / 7 / 11)
per element against float64 with conv_check's derived bar, guard rows around the output and sentinel rows around
the input, and bit for bit against the tiled kernels the same call runs on under conv_cfg 6 (and 5 for k >= 5).

Shapes (B, T, K, dil) are the smallest at which the kernel can go wrong: a window wholly out of range, an
utterance shorter than the halo with both ends in one tile, the 256-row tile edge on either side, a last tile of
one row, two and three tiles, and the halo limit (K - 1) dil = 64.  The epilogue forms are the four stage 0 uses,
with the leaky-ReLU prologue and, for the c2 forms, also without one (how Generator calls c2)."""

import pytest
import torch

import conv_check as CC

pytestmark = pytest.mark.gpu

C = 256
RECORD = dict(BCO=256, BT=256, S=1, SEG=0, nice=1, splits=1, sizeof_in=2, sizeof_compute=2, sizeof_out=2, ROLE=1,
              compute_dtype=1, NI=4, WCO=4)
FORMS = {
    "c1": dict(post=CC.ACT_LRELU, post_slope=0.1),         # post leaky ReLU, no residual, scale 1
    "c2": dict(res1=True),                                 # residual, scale 1
    "last": dict(res1=True, scale=1.0 / 3),                # a chain's last c2 without the MRF accumulator
    "last-acc": dict(res1=True, res2=True, scale=1.0 / 3),  # ... with it
    # c2 as Generator calls it: no prologue activation (c1's epilogue applied c2's leaky ReLU), dilation 1
    "raw-c2": dict(res1=True, pre=CC.ACT_NONE),
    "raw-last-acc": dict(res1=True, res2=True, scale=1.0 / 3, pre=CC.ACT_NONE),
}
FULL = [(2, 40, 11, 5), (3, 257, 7, 1), (2, 300, 3, 5)]    # every form with the leaky-ReLU prologue
ONE = [((1, 1, 7, 3), "last-acc"), ((2, 255, 3, 1), "c1"), ((2, 256, 11, 5), "c2"), ((2, 513, 11, 1), "last"),
       ((1, 257, 3, 32), "last-acc"), ((2, 513, 11, 1), "raw-c2"), ((3, 257, 7, 1), "raw-last-acc"),
       ((2, 300, 3, 1), "raw-last-acc"), ((1, 1, 3, 1), "raw-c2")]
CASES = [(s, f) for s in FULL for f in FORMS if not f.startswith("raw")] + ONE


def _case(shape, form):
    B, T, K, dil = shape
    kw = dict(pre=CC.ACT_LRELU, pre_slope=0.1)
    kw.update(FORMS[form])
    return CC.case(B, T, C, C, K, dil=dil, ydt="bf16", x_rows=3, name=f"plane-{form}_B{B}_T{T}_K{K}_d{dil}", **kw)


@pytest.mark.parametrize("shape,form", CASES, ids=[f"{f}-B{s[0]}-T{s[1]}-K{s[2]}-d{s[3]}" for s, f in CASES])
def test_conv_plane(shape, form):
    from visual_onoma_to_wave_amd import _lib, ops
    c = _case(shape, form)
    m = CC.make(c)
    ref, bar = CC.reference(c, m)
    dev = torch.device("cuda:0")
    x_buf, y_buf = m["x_buf"].to(dev), m["y_buf"].to(dev)
    d = {k: (m[k].to(dev) if m[k] is not None else None) for k in ("w_packed", "bias", "res1", "res2")}
    args = (CC.x_view(c, x_buf), d["w_packed"], d["bias"])

    def kw(yb):
        return dict(out=CC.y_view(c, yb), res1=d["res1"], res2=d["res2"], variant=1, **CC.conv_kwargs(c))

    assert ops.conv1d_plane_takes(*args, **kw(y_buf))
    assert ops.conv1d_plan(*args, **kw(y_buf)) == RECORD
    ops.conv1d(*args, **kw(y_buf))
    assert ops.conv1d_last_launch() == RECORD
    torch.cuda.synchronize()
    int_t = CC._INT[m["x_buf"].dtype]
    assert torch.equal(x_buf.cpu().view(int_t), m["x_buf"].view(int_t)), "the input buffer changed"
    got = y_buf.cpu()
    m["y_buf"].copy_(got)
    CC.verify(c, m, ref, bar)
    # the tiled kernels on the same call: single-role staging (6), and for k >= 5 the role split (5)
    for cfg in (6, 5) if c["K"] >= 5 else (6,):
        y2 = torch.empty_like(y_buf)
        y2.view(int_t).fill_(CC.Y_GUARD[y_buf.dtype])
        _lib.lib().vo_tune(b"conv_cfg", cfg)
        try:
            assert not ops.conv1d_plane_takes(*args, **kw(y2))
            ops.conv1d(*args, **kw(y2))
            assert ops.conv1d_last_launch() == RECORD
            torch.cuda.synchronize()
        finally:
            _lib.lib().vo_tune(b"conv_cfg", 0)
        assert torch.equal(got.view(int_t), y2.cpu().view(int_t)), f"{c['name']}: differs from conv_cfg {cfg}"
