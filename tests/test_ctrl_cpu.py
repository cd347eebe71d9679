"""Tensor-valued energy / duration controls without a GPU: the CPU oracle against the reference's goldens
(tests/golden/make_goldens_ctrl.py), and the host-only ``ops.control_view`` that turns a control into the
(n_control, stride_b, stride_t) of vo_variance_head_ctl."""

import numpy as np
import pytest
import torch

from helpers import golden, rel_l2, stats, t, vtts_arrays
from oracle import acoustic as A
from test_oracle_golden import NAMES, TOL

B, T = 3, 7


@pytest.fixture(scope="module")
def sd():
    return A.complete_state_dict(vtts_arrays(), stats()["energy"])


@pytest.mark.parametrize("tag,shape", [("tok", (2, 5)), ("utt", (2, 1))])
def test_oracle_reproduces_control_goldens(sd, tag, shape):
    g = golden("vtts_inf_ctrl_" + tag)
    assert g["e_control"].shape == shape and g["d_control"].shape == shape
    assert g["e_control"].dtype == np.float32 and g["d_control"].dtype == np.float32
    # the fixture's own margins: no discontinuous step sits where a last-ulp difference could flip it
    assert float(g["d_margin"]) >= 5e-3 and float(g["e_margin"]) >= 5e-4
    if tag == "tok":
        assert (g["d_control"] == 0.0).sum() == 1 and (g["d_control"] == 1.0).sum() == 1
    sd2 = dict(sd)
    key = "variance_adaptor.duration_predictor.linear_layer.bias"
    sd2[key] = sd[key] + float(g["dur_bias_shift"])
    out = A.vtts_forward(sd2, t(g["in_audiotypes"]), t(g["in_texts"]), t(g["in_src_lens"]), int(g["in_max_src_len"]),
                         images=t(g["in_images"]), energy_stats=stats()["energy"], e_control=t(g["e_control"]),
                         d_control=t(g["d_control"]))
    for n, o in zip(NAMES, out):
        if o is None:
            assert n not in g
        elif o.dtype in (torch.bool, torch.int64) or n == "d_rounded":
            np.testing.assert_array_equal(o.numpy(), g[n], err_msg=n)
        else:
            assert rel_l2(o, g[n]) < TOL, n


def _views():
    """name -> (control tensor, expected (n_control, stride_b, stride_t)) at B = 3, T = 7."""
    base = torch.arange(B * 14, dtype=torch.float32)
    return {
        "0-d": (base[4], (1, 0, 0)),
        "(1,)": (base[:1], (1, 0, 0)),
        "(T,)": (base[:T], (T, 0, 1)),
        "(1,T)": (base[:T].reshape(1, T), (T, 0, 1)),
        "(B,1)": (base[:B].reshape(B, 1), (B, 1, 0)),
        "(B,T)": (base[:B * T].reshape(B, T), (B * T, T, 1)),
        "(T,B).T": (base[:B * T].reshape(T, B).T, ((B - 1) + (T - 1) * B + 1, 1, B)),
        "(B,14)[:,::2]": (base.reshape(B, 14)[:, ::2], ((B - 1) * 14 + (T - 1) * 2 + 1, 14, 2)),
    }


@pytest.mark.parametrize("name", list(_views()))
def test_control_view_strides_and_extent(name):
    from visual_onoma_to_wave_amd import ops
    c, want = _views()[name]
    out, n, sb, st = ops.control_view(c, B, T)
    assert (n, sb, st) == want
    # an fp32 tensor goes through as it is: same memory, nothing materialised
    assert out.dtype == torch.float32 and out.data_ptr() == c.data_ptr()
    # the strides address the broadcast values, and the last token is the last float of the extent
    flat = torch.as_strided(out, (n,), (1,))
    ref = torch.broadcast_to(c, (B, T))
    for b in range(B):
        for tt in range(T):
            assert flat[b * sb + tt * st] == ref[b, tt]
    assert (B - 1) * sb + (T - 1) * st == n - 1


@pytest.mark.parametrize("shape", [(3,), (2, 7), (3, 7, 1), (0,), (3, 0)])
def test_control_view_refuses_shapes(shape):
    from visual_onoma_to_wave_amd import ops
    with pytest.raises(ValueError, match=r"\(3, 7\)") as e:
        ops.control_view(torch.zeros(shape), B, T)
    assert str(shape) in str(e.value)  # both shapes are named


@pytest.mark.parametrize("make", [lambda: torch.arange(7, dtype=torch.int64), lambda: torch.ones(3, 1, dtype=torch.float64),
                                  lambda: torch.ones(3, 7, dtype=torch.bfloat16), lambda: np.full((1, 7), 1.5),
                                  lambda: [[0.5], [1.0], [2.0]]], ids=["int64", "fp64", "bf16", "numpy", "list"])
def test_control_view_converts_to_fp32(make):
    from visual_onoma_to_wave_amd import ops
    c = make()
    out, n, sb, st = ops.control_view(c, B, T)
    assert out.dtype == torch.float32
    ref = torch.broadcast_to(torch.as_tensor(np.asarray(c.float() if torch.is_tensor(c) else c)).float(), (B, T))
    assert torch.equal(out.expand(B, T), ref)
    assert (sb, st) == out.expand(B, T).stride() and n == (B - 1) * sb + (T - 1) * st + 1


@pytest.mark.parametrize("args,word", [((None, 21, 7, 1), "null control"), ((0x1000, 21, -7, 1), "negative stride"),
                                       ((0x1000, 21, 7, -1), "negative stride"), ((0x1000, 20, 7, 1), "reaches past"),
                                       ((0x1000, 2, 1, 0), "reaches past"), ((0x1000, 1 << 62, 1 << 40, 1), "reaches past")])
def test_entry_refuses_on_the_host(args, word):
    """vo_variance_head_ctl checks its control view before anything touches the device: VO_ERR_INVALID with a
    message, for pointers that are never dereferenced (0x1000 stands for device memory)."""
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    d = _lib.HeadDesc()
    d.kind = _lib.HEAD_DURATION
    d.h = d.w = d.pred = 0x1000
    d.B, d.T, d.D = B, T, 256
    assert L.vo_variance_head_ctl(d, *args, None) == -1
    assert word in L.vo_last_error().decode()


def test_python_numbers_are_not_tensor_controls():
    """Numbers keep the scalar entry (the descriptor's float fields); everything else is a tensor control."""
    from visual_onoma_to_wave_amd import ops
    for c in (1, 1.5, np.float32(0.5), np.int64(2)):
        assert ops._is_number(c)
    for c in (torch.tensor(1.5), np.ones(1), [1.0]):
        assert not ops._is_number(c)
