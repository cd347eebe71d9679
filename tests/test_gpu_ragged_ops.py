"""Ragged batches, one op at a time (include/vonoma.h, "per-utterance lengths").

Every case runs a batch of B = 5 utterances of lengths {T, BT + 1, BT, 1, 0} rows (lens_scale = 1), BT the kernel's
rows per tile and T at least three tiles plus a remainder; the input rows, and the MRF-accumulator rows, past an
utterance's end hold NaN and the output is pre-filled with a sentinel.  Asserted, bit for bit:
  * rows < R_b equal the dense op on x[b:b+1, :R_b] alone, and none is NaN;
  * rows >= R_b still hold the sentinel (conv_post: exactly 0);
  * every length = T equals the dense call on the batch; every length = 0 writes nothing.
conv1d picks its tile from the shape, so the dense call on one utterance may run another tile than the batch: the
test asserts that the two vo_conv1d_last_launch records are equal for the lengths T, BT + 1 and BT (B and T are chosen
so that they are).  The one-row utterance alone cannot share the batch's tile (the dispatcher sends T_out <= 16 to
its 16-row tiles whatever B is, and the fp32 ones sum in another order), so there the dense op runs on the utterance
followed by zero rows up to BT + 1 rows: for a single conv, rows that are zero are the conv's own zero padding (the
leaky ReLU of 0 is 0), so its rows < R_b are those of the dense op on x[b:b+1, :R_b], on the batch's tile -- the
records are asserted equal there too, and the comparison stays bit for bit.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 5
NAN = float("nan")


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _rand(shape, seed, dtype=torch.bfloat16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _conv_w(Co, Ci, K, seed, dtype):
    from visual_onoma_to_wave_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Co, Ci, K, generator=g) * (1.0 / (Ci * K) ** 0.5)
    return ops.pack_conv_weight(w.cuda(), dtype), (torch.randn(Co, generator=g) * 0.1).cuda()


def run_case(op, x, BT, up=1, acc=None, zero_tail=False, record=None):
    """op(x, lens, out, acc) -> out; lens None = the dense op (out None: a fresh output).  ``up``: output rows per
    input row.  ``record`` (conv1d): returns the launch record of the call just made."""
    T = x.shape[1]
    assert x.shape[0] == B and T >= 3 * BT + 1, (x.shape, BT)
    lens_list = [T, BT + 1, BT, 1, 0]
    ref_full = op(x, None, None, acc)
    rec_dense_batch = record() if record else None
    sent = torch.full_like(ref_full, 0.0 if zero_tail else -7.5)
    xn = x.clone()
    accn = None if acc is None else acc.clone()
    for b, R in enumerate(lens_list):
        xn[b, R:] = NAN
        if accn is not None:
            accn[b, R * up:] = NAN
    got = op(xn, _lens(lens_list), None if zero_tail else sent.clone(), accn)
    rec = record() if record else None
    torch.cuda.synchronize()
    if record:
        assert rec == rec_dense_batch and rec["BT"] == BT, (rec, rec_dense_batch, BT)
    for b, R in enumerate(lens_list):
        Ro = R * up
        assert torch.equal(got[b, Ro:], sent[b, Ro:]), f"utterance {b}: rows >= {Ro} were written"
        if R == 0:
            continue
        if record and R < BT:  # conv1d, an utterance shorter than a tile: zero rows up to BT + 1 (module docstring)
            xa = torch.zeros((1, BT + 1) + x.shape[2:], dtype=x.dtype, device=x.device)
            xa[0, :R] = x[b, :R]
            aa = None
            if acc is not None:
                aa = torch.zeros((1, (BT + 1) * up) + acc.shape[2:], dtype=acc.dtype, device=acc.device)
                aa[0, :Ro] = acc[b, :Ro]
            alone = op(xa, None, None, aa)[:, :Ro]
        else:
            alone = op(x[b:b + 1, :R].contiguous(), None, None, None if acc is None else acc[b:b + 1, :Ro].contiguous())
        if record:
            assert record() == rec, (R, record(), rec)
        assert not torch.isnan(got[b, :Ro].float()).any(), f"utterance {b}: NaN in its valid rows"
        assert torch.equal(got[b, :Ro], alone[0]), f"utterance {b} (R = {R}) differs from the dense op on it alone"
    # every length = T: the dense call; every length = 0: nothing is written
    full = op(x, _lens([T] * B), None if zero_tail else sent.clone(), acc)
    assert torch.equal(full, ref_full)
    none = op(torch.full_like(x, NAN), _lens([0] * B), None if zero_tail else sent.clone(),
              None if acc is None else torch.full_like(acc, NAN))
    torch.cuda.synchronize()
    assert torch.equal(none, sent)


# ------------------------------------------------------------------------------ fused pairs and k = 3 blocks

def _pair_bt(C, K):
    # mrf_pair_kernel C = 32: 512 c1 rows per tile; the plane kernel: 512 (C = 64) / 256 (C = 128); less the K - 1 halo
    return (256 if C == 128 else 512) - (K - 1)


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("C,K,dil,frag", [(32, 7, 3, False), (32, 11, 5, False), (64, 7, 1, False), (64, 11, 5, False),
                                          (128, 7, 5, False), (128, 11, 3, False), (64, 7, 3, True), (64, 11, 1, True),
                                          (128, 7, 1, True), (128, 11, 5, True)])
def test_resblock_pair_ragged(C, K, dil, frag, with_acc):
    from visual_onoma_to_wave_amd import ops
    BT = _pair_bt(C, K)
    T = 3 * BT + 37
    (w1, b1), (w2, b2) = _conv_w(C, C, K, 1, torch.bfloat16), _conv_w(C, C, K, 2, torch.bfloat16)
    if frag:
        w1, w2 = ops.pack_frag(w1), ops.pack_frag(w2)
    x = _rand((B, T, C), 3)
    acc = _rand((B, T, C), 4) if with_acc else None

    def op(x, lens, out, acc):
        return ops.resblock_pair(x, w1, b1, w2, b2, K, dil, 0.1, out=out, out_scale=1.0 / 3 if acc is not None else 1.0,
                                 acc=acc, frag=frag, lens=lens)
    run_case(op, x, BT, acc=acc)


@pytest.mark.parametrize("C,BT", [(32, 104), (64, 488), (128, 200)])  # tests/test_gpu_parity.py: output rows per tile
def test_resblock3_ragged(C, BT):
    from visual_onoma_to_wave_amd import ops
    T = 3 * BT + 29
    ws = [_conv_w(C, C, 3, 10 + i, torch.bfloat16) for i in range(6)]
    w1s, b1s = [w for w, _ in ws[:3]], [b for _, b in ws[:3]]
    w2s, b2s = [w for w, _ in ws[3:]], [b for _, b in ws[3:]]
    x, acc = _rand((B, T, C), 5), _rand((B, T, C), 6)

    def op(x, lens, out, acc):
        return ops.resblock3(x, w1s, b1s, w2s, b2s, (1, 3, 5), 0.1, out=out, out_scale=1.0 / 3, acc=acc, lens=lens)
    run_case(op, x, BT, acc=acc)
    run_case(lambda x, lens, out, acc: ops.resblock3(x, w1s, b1s, w2s, b2s, (1, 3, 5), 0.1, out=out, lens=lens), x, BT)


@pytest.mark.parametrize("C,K", [(64, 7), (128, 11), (64, 3), (128, 3)])
def test_plane_kernels_ragged_with_epilogue_accumulate(C, K):
    """An out_scale whose inverse is no bf16 value (0.3): the plane kernels then add the MRF accumulator in their
    epilogue (mrf_acc_mode 1), not through the identity MFMA the 1/3 of the vocoder takes -- instantiations of their own."""
    from visual_onoma_to_wave_amd import ops
    BT = _pair_bt(C, K) if K > 3 else {64: 488, 128: 200}[C]
    T = 3 * BT + 13
    x, acc = _rand((B, T, C), 60), _rand((B, T, C), 61)
    if K > 3:
        (w1, b1), (w2, b2) = _conv_w(C, C, K, 1, torch.bfloat16), _conv_w(C, C, K, 2, torch.bfloat16)
        run_case(lambda x, lens, out, acc: ops.resblock_pair(x, w1, b1, w2, b2, K, 3, 0.1, out=out, out_scale=0.3, acc=acc,
                                                             lens=lens), x, BT, acc=acc)
    else:
        ws = [_conv_w(C, C, 3, 10 + i, torch.bfloat16) for i in range(6)]
        w1s, b1s, w2s, b2s = ([w for w, _ in ws[:3]], [b for _, b in ws[:3]], [w for w, _ in ws[3:]],
                              [b for _, b in ws[3:]])
        run_case(lambda x, lens, out, acc: ops.resblock3(x, w1s, b1s, w2s, b2s, (1, 3, 5), 0.1, out=out, out_scale=0.3,
                                                         acc=acc, lens=lens), x, BT, acc=acc)


# ------------------------------------------------------------------------------ streaming upsamplers

# the three shapes of vo_ups_takes (upsample.hip): (Ci, C_out, stride) and the input steps per unit, 16 NJ
@pytest.mark.parametrize("Ci,cout,u,BT", [(128, 64, 2, 64), (64, 32, 2, 64), (256, 128, 8, 16)])
def test_streaming_upsampler_ragged(Ci, cout, u, BT):
    from visual_onoma_to_wave_amd import ops
    T = 3 * BT + 11
    g = torch.Generator().manual_seed(7)
    wt = torch.randn(Ci, cout, 2 * u, generator=g) * (1.0 / Ci ** 0.5)
    w = ops.pack_conv_weight(wt.cuda(), torch.bfloat16, transposed_stride=u)
    bias = (torch.randn(cout, generator=g) * 0.1).cuda()
    x = _rand((B, T, Ci), 8)

    def op(x, lens, out, acc):
        y = ops.conv1d(x, w, bias, Co=u * cout, K=2, pad=1, pre_act=ops.ACT_LRELU, pre_slope=0.1, out=out,
                       transposed=dict(stride=u, pad=u // 2, cout=cout), out_dtype=torch.bfloat16, lens=lens)
        assert all(v == 0 for v in ops.conv1d_last_launch().values()), "not the streaming upsampler"
        return y
    run_case(op, x, BT, up=u)


# ------------------------------------------------------------------------------ conv1d (the tiled kernel)

def _rec():
    from visual_onoma_to_wave_amd import ops
    return ops.conv1d_last_launch()


def _conv1d(*args, **kw):
    """ops.conv1d; the plan of the same arguments (ops.conv1d_plan: no launch) must be the record the launch left,
    and must leave that record alone."""
    from visual_onoma_to_wave_amd import ops
    y = ops.conv1d(*args, **kw)
    rec = _rec()
    assert ops.conv1d_plan(*args, **kw) == rec and _rec() == rec, (ops.conv1d_plan(*args, **kw), rec)
    return y


def _first_bt(op, x):
    op(x, None, None, None)
    return _rec()["BT"]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_conv_pre_ragged(dt):
    """conv_pre (80 -> 512, k7) reading an fp32 mel, as Generator.run calls it."""
    from visual_onoma_to_wave_amd import ops
    w, bias = _conv_w(512, 80, 7, 20, dt)
    T = 3 * 64 + 5  # B * T <= 2048 rows: the 64 x 64 tile, for the batch and for an utterance alone
    x = _rand((B, T, 80), 21, torch.float32)

    def op(x, lens, out, acc):
        return _conv1d(x, w, bias, Co=512, K=7, pad=3, out=out, out_dtype=dt, compute_dtype=dt, lens=lens)
    assert _first_bt(op, x) == 64
    run_case(op, x, 64, record=_rec)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_ups0_ragged(dt):
    """ups0 (512 -> 256, k16 s8) in its polyphase form on the tiled conv: R_b + 1 phase rows, 8 R_b output rows."""
    from visual_onoma_to_wave_amd import ops
    g = torch.Generator().manual_seed(22)
    wt = torch.randn(512, 256, 16, generator=g) * (1.0 / 512 ** 0.5)
    w = ops.pack_conv_weight(wt.cuda(), dt, transposed_stride=8)
    bias = (torch.randn(256, generator=g) * 0.1).cuda()
    T = 3 * 64 + 5
    x = _rand((B, T, 512), 23, dt)

    def op(x, lens, out, acc):
        return _conv1d(x, w, bias, Co=8 * 256, K=2, pad=1, pre_act=ops.ACT_LRELU, pre_slope=0.1, out=out,
                       transposed=dict(stride=8, pad=4, cout=256), out_dtype=dt, compute_dtype=dt, lens=lens)
    assert _first_bt(op, x) == 64
    run_case(op, x, 64, up=8, record=_rec)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K,dil", [(3, 1), (3, 5), (7, 1), (7, 5), (11, 1), (11, 5)])
def test_stage0_conv_ragged(K, dil, dt):
    """The MRF stage-0 convs (C = 256, variant 1: their own 256 x 256 instantiation in bf16) with both residuals:
    y = (conv(lrelu x) + res1) / 3 + res2."""
    from visual_onoma_to_wave_amd import ops
    w, bias = _conv_w(256, 256, K, 30 + K, dt)
    BT = 256 if dt == torch.bfloat16 else 64
    T = 3 * BT + 5
    x, res1, res2 = _rand((B, T, 256), 31, dt), _rand((B, T, 256), 32, dt), _rand((B, T, 256), 33, dt)

    def op(x, lens, out, acc):
        # acc carries both residuals, so that run_case cuts / poisons them with the input
        r1, r2 = acc[..., :256].contiguous(), acc[..., 256:].contiguous()
        return _conv1d(x, w, bias, Co=256, K=K, dil=dil, pad=dil * (K - 1) // 2, pre_act=ops.ACT_LRELU, pre_slope=0.1,
                       res1=r1, res2=r2, out=out, out_scale=1.0 / 3, compute_dtype=dt, out_dtype=dt, variant=1,
                       lens=lens)
    both = torch.cat([res1, res2], dim=-1)
    op(x, None, None, both)
    assert _rec()["BT"] == BT and _rec()["ROLE"] == (1 if dt == torch.bfloat16 else 0)
    run_case(op, x, BT, acc=both, record=_rec)


# ------------------------------------------------------------------------------ conv_post

@pytest.mark.parametrize("dt,C,BT", [(torch.bfloat16, 32, 250), (torch.float32, 32, 256), (torch.bfloat16, 64, 256)])
def test_conv_post_ragged(dt, C, BT):
    """Both kernels: one input row per thread (bf16, C = 32, k7: 250 outputs per workgroup) and the LDS stencil (256)."""
    from visual_onoma_to_wave_amd import ops
    g = torch.Generator().manual_seed(40)
    wk = (torch.randn(7, C, generator=g) * 0.05).cuda()
    T = 3 * BT + 9
    x = _rand((B, T, C), 41, dt)
    run_case(lambda x, lens, out, acc: ops.conv_post(x, wk, 0.03, slope=0.01, lens=lens)[..., None], x, BT,
             zero_tail=True)


# ------------------------------------------------------------------------------ what a ragged call refuses

def _pair_inputs(C=64, K=7, T=64):
    (w1, b1), (w2, b2) = _conv_w(C, C, K, 1, torch.bfloat16), _conv_w(C, C, K, 2, torch.bfloat16)
    return _rand((B, T, C), 3), w1, b1, w2, b2


def test_ragged_conv1d_refuses_what_the_vocoder_does_not_reach():
    from visual_onoma_to_wave_amd import ops
    lens = _lens([40, 30, 20, 10, 0])
    w, bias = _conv_w(64, 64, 3, 50, torch.bfloat16)
    x = _rand((B, 40, 64), 51)
    kw = dict(Co=64, K=3, pad=1, lens=lens)
    ops.conv1d(x, w, bias, **kw)  # the supported form runs
    with pytest.raises(RuntimeError, match="stride"):
        ops.conv1d(x, w, bias, stride=2, **kw)
    with pytest.raises(RuntimeError, match="stride|groups"):
        ops.conv1d(x, w, bias, groups=2, **kw)
    with pytest.raises(RuntimeError, match="ymask"):
        ops.conv1d(x, w, None, ymask=torch.ones(B, 40, 64, dtype=torch.bfloat16, device="cuda"), ymask_slope=0.1, **kw)
    with pytest.raises(RuntimeError, match="same-length"):
        ops.conv1d(x, w, bias, Co=64, K=3, pad=0, lens=lens)
    wf, bf = _conv_w(64, 64, 3, 52, torch.float32)
    xf = _rand((B, 40, 64), 53, torch.float32)
    with pytest.raises(RuntimeError, match="F32X3"):
        ops.conv1d(xf, wf, bf, compute_dtype=ops.F32X3, **kw)
    with pytest.raises(RuntimeError, match="utterance-segment"):  # fp32 at T_out <= 16: SEG tiles
        ops.conv1d(xf[:, :12].contiguous(), wf, bf, compute_dtype=torch.float32, **kw)
    # a split-reduction workspace (ops.conv1d never passes one with lens: straight through the C ABI)
    import ctypes
    from visual_onoma_to_wave_amd import _lib
    y = torch.empty(B, 40, 64, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    d = _lib.Conv1dDesc()
    d.x, d.x_dtype, d.x_bstride, d.ldx = x.data_ptr(), _lib.VO_BF16, 40 * 64, 64
    d.w, d.bias, d.y, d.y_dtype, d.y_bstride, d.ldy = w.data_ptr(), bias.data_ptr(), y.data_ptr(), _lib.VO_BF16, 40 * 64, 64
    d.B, d.T_in, d.T_out, d.Ci, d.Co, d.K, d.dil, d.pad = B, 40, 40, 64, 64, 3, 1, 1
    d.out_scale, d.compute_dtype = 1.0, _lib.VO_BF16
    d.lens, d.lens_scale = lens.data_ptr(), 1
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    assert _lib.lib().vo_conv1d(ctypes.byref(d), None) != 0
    assert b"workspace" in _lib.lib().vo_last_error()
    torch.cuda.synchronize()


def test_ragged_lens_validation():
    from visual_onoma_to_wave_amd import ops
    x, w1, b1, w2, b2 = _pair_inputs()
    with pytest.raises(TypeError):
        ops.resblock_pair(x, w1, b1, w2, b2, 7, 1, lens=torch.zeros(B, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.resblock_pair(x, w1, b1, w2, b2, 7, 1, lens=_lens([1, 2, 3]))
    with pytest.raises(ValueError):
        ops.resblock_pair(x, w1, b1, w2, b2, 7, 1, lens=torch.zeros(B, dtype=torch.int32))  # on the host
    with pytest.raises(ValueError):
        ops.resblock_pair(x, w1, b1, w2, b2, 7, 1, lens=_lens([1] * B), lens_scale=0)
    with pytest.raises(RuntimeError, match="K=3"):  # k = 3 pairs run as resblock3 in the vocoder
        (w31, b31), (w32, b32) = _conv_w(64, 64, 3, 1, torch.bfloat16), _conv_w(64, 64, 3, 2, torch.bfloat16)
        ops.resblock_pair(x, w31, b31, w32, b32, 3, 1, lens=_lens([1] * B))


@pytest.mark.parametrize("knob,value", [("pair_cfg", 93), ("rb3_cfg", 80), ("ups_cfg", 2), ("conv_cfg", 6)])
def test_knob_without_ragged_kernel_is_an_error(knob, value):
    """A vo_tune value that selects a kernel with no ragged form is refused by name, not run dense."""
    from visual_onoma_to_wave_amd import _lib, ops
    lens = _lens([64, 50, 30, 1, 0])
    L = _lib.lib()
    assert L.vo_tune(knob.encode(), value) == 0
    try:
        with pytest.raises(RuntimeError, match=knob):
            if knob == "pair_cfg":
                x, w1, b1, w2, b2 = _pair_inputs()
                ops.resblock_pair(x, w1, b1, w2, b2, 7, 1, lens=lens)
            elif knob == "rb3_cfg":
                ws = [_conv_w(32, 32, 3, 10 + i, torch.bfloat16) for i in range(6)]
                ops.resblock3(_rand((B, 64, 32), 5), [w for w, _ in ws[:3]], [b for _, b in ws[:3]],
                              [w for w, _ in ws[3:]], [b for _, b in ws[3:]], (1, 3, 5), lens=lens)
            elif knob == "ups_cfg":
                g = torch.Generator().manual_seed(7)
                w = ops.pack_conv_weight((torch.randn(128, 64, 4, generator=g) * 0.1).cuda(), torch.bfloat16,
                                         transposed_stride=2)
                ops.conv1d(_rand((B, 64, 128), 8), w, None, Co=128, K=2, pad=1, lens=lens,
                           transposed=dict(stride=2, pad=1, cout=64))
            else:
                w, bias = _conv_w(256, 256, 3, 30, torch.bfloat16)
                ops.conv1d(_rand((B, 64, 256), 31), w, bias, Co=256, K=3, pad=1, variant=1, lens=lens)
    finally:
        assert L.vo_tune(knob.encode(), 0) == 0
    torch.cuda.synchronize()
