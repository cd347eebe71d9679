"""vo_conv_post_pcm16 / vo_conv_post_pcm16_lens: the conv_post kernels with an int16 output element.

The reference is ``ops.conv_post`` (the fp32 instantiation of the same kernel) on the same tensors, fed through
``pcm_check.check_pcm``.  Shapes sit at the tile edges of both kernels (250 outputs per workgroup in the rows
kernel, 256 rows in the stencil kernel; odd T makes the rows of y 2-byte aligned only); every output lies in a
buffer followed by 64 guard elements of 0x5A5A."""

import ctypes

import numpy as np
import pytest
import torch

import pcm_check as PC

pytestmark = pytest.mark.gpu

SCALES = (32768.0, 32767.0)  # the second is no power of two: it pins the fp32 product
ROWS_T = (249, 250, 251, 501)
STENCIL_T = (255, 256, 257)
STENCIL = (("bf16", 32, 5), ("bf16", 64, 7), ("f32", 32, 7))
CASES = [PC.post_case("bf16", 32, 7, T) for T in ROWS_T] + \
        [PC.post_case(dt, C, K, T) for dt, C, K in STENCIL for T in STENCIL_T]
RAGGED = [PC.post_case("bf16", 32, 7, 251), PC.post_case("bf16", 32, 7, 501), PC.post_case("bf16", 32, 5, 257),
          PC.post_case("f32", 32, 7, 257)]
VO_ERR_INVALID = -1
SLOPE = 0.01


def _dev(c, x, w):
    return x.to(torch.bfloat16 if c["dt"] == "bf16" else torch.float32).cuda().contiguous(), w.cuda().contiguous()


def _pcm(x, w, bias, scale, lens=None, lens_scale=1, buf=None):
    """The C entry on a guarded buffer: (return code, the buffer on the host)."""
    from visual_onoma_to_wave_amd import _lib, ops
    B, T, C = x.shape
    if buf is None:
        buf = torch.from_numpy(PC.guarded(B, T)).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    if lens is None:
        rc = L.vo_conv_post_pcm16(p(x), ops.vo_dtype(x), p(w), bias, B, T, C, w.shape[0], SLOPE, scale, p(buf), st)
    else:
        rc = L.vo_conv_post_pcm16_lens(p(x), ops.vo_dtype(x), p(w), bias, B, T, C, w.shape[0], SLOPE, scale, p(buf),
                                       st, p(lens), lens_scale)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_pcm_dense(c, scale):
    from visual_onoma_to_wave_amd import ops
    x, w, bias = PC.post_operands(c)
    x, w = _dev(c, x, w)
    ref = ops.conv_post(x, w, bias, slope=SLOPE).cpu().numpy()
    rc, buf = _pcm(x, w, bias, scale)
    assert rc == 0
    frac = PC.check_pcm(buf, ref, scale, name=c["name"])
    print(f"{c['name']} scale {scale}: band fraction {frac:.3f}, peak |y| {np.abs(ref).max():.3f}")
    # the Python front end returns the same samples
    q = ops.conv_post(x, w, bias, slope=SLOPE, pcm_scale=scale)
    assert q.dtype == torch.int16 and q.shape == ref.shape
    np.testing.assert_array_equal(q.cpu().numpy(), PC.split_guard(buf, *ref.shape)[0])


def _ragged(c, rows, lens_scale, scale):
    from visual_onoma_to_wave_amd import ops
    x, w, bias = PC.post_operands(c, seed=1)
    B, T = c["B"], c["T"]
    for b, r in enumerate(rows):
        x[b, min(max(r * lens_scale, 0), T):] = float("nan")  # nothing may read the padded rows
    x, w = _dev(c, x, w)
    lens = torch.tensor(rows, dtype=torch.int32, device="cuda")
    ref = ops.conv_post(x, w, bias, slope=SLOPE, lens=lens, lens_scale=lens_scale).cpu().numpy()
    valid = [min(max(r * lens_scale, 0), T) for r in rows]
    for b, r in enumerate(valid):
        assert np.isfinite(ref[b]).all() and not ref[b, r:].any()
    rc, buf = _pcm(x, w, bias, scale, lens=lens, lens_scale=lens_scale)
    assert rc == 0
    PC.check_pcm(buf, ref, scale, rows=valid, name=f"{c['name']}-rows{tuple(rows)}")
    q = ops.conv_post(x, w, bias, slope=SLOPE, lens=lens, lens_scale=lens_scale, pcm_scale=scale)
    np.testing.assert_array_equal(q.cpu().numpy(), PC.split_guard(buf, B, T)[0])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("c", RAGGED, ids=[c["name"] for c in RAGGED])
def test_pcm_ragged(c, scale):
    _ragged(c, (0, 1, 250), 1, scale)
    _ragged(c, (251, c["T"], c["T"] + 5), 1, scale)


@pytest.mark.parametrize("dt,C,K", [("bf16", 32, 7), ("f32", 32, 7)])
def test_pcm_ragged_lens_scale_256(dt, C, K):
    _ragged(PC.post_case(dt, C, K, 512), (2, 1, 0), 256, 32768.0)


@pytest.mark.parametrize("c", [PC.post_case("bf16", 32, 7, 251), PC.post_case("f32", 32, 7, 257)],
                         ids=["rows", "stencil"])
def test_pcm_saturates_instead_of_wrapping(c):
    """tanhf gives exactly +-1.0f for large sums: 1.0 * 32768 is outside int16 and stores 32767 (the host cast
    wraps to -32768); the negative end is in range."""
    from visual_onoma_to_wave_amd import ops
    x, w, bias = PC.post_operands(c, seed=2)
    w = w.abs() * 400.0
    x[0] = x[0].abs() + 0.5
    x[1] = -(x[1].abs() + 0.5)  # through the 0.01 leaky slope: still a sum below -20
    xd, wd = _dev(c, x, w)
    ref = ops.conv_post(xd, wd, bias, slope=SLOPE).cpu().numpy()
    assert (ref[0] == np.float32(1.0)).all() and (ref[1] == np.float32(-1.0)).all()
    for scale, hi, lo in ((32768.0, 32767, -32768), (32767.0, 32767, -32767)):
        rc, buf = _pcm(xd, wd, bias, scale)
        assert rc == 0
        PC.check_guard(buf, c["B"], c["T"])
        q = PC.split_guard(buf, c["B"], c["T"])[0]
        assert (q[0] == hi).all() and (q[1] == lo).all(), (scale, q[0, :4], q[1, :4])
        np.testing.assert_array_equal(q[:2], PC.expected_pcm(ref[:2], scale))
        assert np.abs(q[2].astype(np.int32) - PC.expected_pcm(ref[2], scale).astype(np.int32)).max() <= 1


@pytest.mark.parametrize("c", [PC.post_case("bf16", 32, 7, 501), PC.post_case("bf16", 64, 7, 257)],
                         ids=["rows", "stencil"])
def test_pcm_nan_stores_zero(c):
    from visual_onoma_to_wave_amd import ops
    x, w, bias = PC.post_operands(c, seed=3)
    x[1, 100:110] = float("nan")
    xd, wd = _dev(c, x, w)
    ref = ops.conv_post(xd, wd, bias, slope=SLOPE).cpu().numpy()
    nan = np.isnan(ref)
    assert nan[1, 100:110].all() and 10 <= nan.sum() <= 10 + c["K"] - 1 and not nan[[0, 2]].any()
    rc, buf = _pcm(xd, wd, bias, 32768.0)
    assert rc == 0
    PC.check_pcm(buf, ref, 32768.0, name=c["name"])
    assert not PC.split_guard(buf, c["B"], c["T"])[0][nan].any()


def test_pcm_refusals_launch_nothing():
    from visual_onoma_to_wave_amd import _lib, ops
    c = PC.post_case("bf16", 32, 7, 251)
    x, w, bias = PC.post_operands(c)
    xd, wd = _dev(c, x, w)
    lens = torch.tensor([3, 2, 1], dtype=torch.int32, device="cuda")
    for scale in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        for ln in (None, lens):
            rc, buf = _pcm(xd, wd, bias, scale, lens=ln)
            assert rc == VO_ERR_INVALID, scale
            assert b"scale" in _lib.lib().vo_last_error()
            assert (buf == PC.GUARD_VALUE).all(), "a refused call wrote to the output"
        with pytest.raises(RuntimeError, match="scale"):
            ops.conv_post(xd, wd, bias, pcm_scale=scale)
    # what vo_conv_post refuses: C = 12, an even K, a slope outside [0, 1]
    x12 = torch.zeros(3, 251, 12, dtype=torch.bfloat16, device="cuda")
    w12 = torch.zeros(7, 12, device="cuda")
    rc, buf = _pcm(x12, w12, bias, 32768.0)
    assert rc == VO_ERR_INVALID and b"C=12" in _lib.lib().vo_last_error() and (buf == PC.GUARD_VALUE).all()
    rc, buf = _pcm(x12, w12, bias, 32768.0, lens=lens)
    assert rc == VO_ERR_INVALID and (buf == PC.GUARD_VALUE).all()
    rc, buf = _pcm(xd, wd[:6].contiguous(), bias, 32768.0)
    assert rc == VO_ERR_INVALID and (buf == PC.GUARD_VALUE).all()
    rc, buf = _pcm(xd, wd, bias, 32768.0, lens=lens, lens_scale=0)
    assert rc == VO_ERR_INVALID and (buf == PC.GUARD_VALUE).all()
