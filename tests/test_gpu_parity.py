"""GPU parity: the HIP path vs the golden vectors (reference outputs) and vs the CPU oracle.

Tolerances (relative L2 unless stated):
  * fp32 mode (exact-f32 MFMA; only summation order differs from oneDNN):  2e-5 per
    module, 1e-4 for whole-model outputs;
  * bf16 kernels (bf16 operands, fp32 accumulation):  1e-2 (measured reference-vs-
    reference bf16 drift is 3.4e-3 for the Generator, 4.5e-3 for vTTS);
  * integer / index results (LengthRegulator frames + mel_len, bucket indices, masks,
    d_rounded):  bit-exact.
"""

import numpy as np

import pytest
import torch

from helpers import configs, golden, hifigan_arrays, hifigan_h, rel_l2, stats, vtts_arrays
from weights import load_into

pytestmark = pytest.mark.gpu

F32_MOD, F32_MODEL, BF16 = 2e-5, 1e-4, 1e-2


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.fixture(scope="module")
def vtts(device):
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    return m.to(device).eval()


@pytest.fixture(scope="module")
def gen(device):
    from visual_onoma_to_wave_amd import hifigan
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    return g.to(device)


def _prec(m, mode):
    m.set_precision(mode)
    return torch.float32 if mode == "fp32" else torch.bfloat16


# ------------------------------------------------------------------------------ acoustic modules

@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, BF16)])
def test_vfe(vtts, dt, tol):
    g = golden("vfe")
    vfe = vtts.encoder.VisualFeatureExtractor
    vfe.set_compute_dtype(dt)
    with torch.no_grad():
        out = vfe(cuda(g["images"]))
    assert rel_l2(out.float().cpu(), g["out"]) < tol


@pytest.mark.parametrize("name,which", [("fft_enc", "encoder"), ("fft_dec", "decoder")])
@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, BF16)])
def test_fft_block(vtts, name, which, dt, tol):
    from visual_onoma_to_wave_amd.utils.tools import get_mask_from_lengths
    g = golden(name)
    layer = getattr(vtts, which).layer_stack[0]
    layer.set_compute_dtype(dt)
    L = g["x"].shape[1]
    mask = get_mask_from_lengths(cuda(g["lens"]), L)
    with torch.no_grad():
        out, _ = layer(cuda(g["x"]), mask=mask)
    assert rel_l2(out.float().cpu(), g["out"]) < tol


def test_variance_predictors(vtts):
    from visual_onoma_to_wave_amd.utils.tools import get_mask_from_lengths
    g = golden("var_pred")
    va = vtts.variance_adaptor
    va.set_compute_dtype(torch.float32)
    mask = get_mask_from_lengths(cuda(g["lens"]), 12)
    with torch.no_grad():
        ld = va.duration_predictor(cuda(g["x"]), mask)
        en = va.energy_predictor(cuda(g["x"]), mask)
    assert rel_l2(ld.cpu(), g["log_d"]) < F32_MOD
    assert rel_l2(en.cpu(), g["energy"]) < F32_MOD
    assert (ld.cpu().numpy()[1, 5:] == 0).all()


def test_energy_bucketize_embed_exact(vtts):
    from visual_onoma_to_wave_amd import ops
    g = golden("bucketize")
    va = vtts.variance_adaptor
    vals = cuda(g["values"]).reshape(1, -1)
    n = vals.shape[1]
    h = torch.zeros((1, n, 256), device="cuda")
    x = torch.zeros((1, n, 256), device="cuda")
    _, idx = ops.energy_head(h, torch.zeros(256, device="cuda"), 0.0, None, x,
                             va.energy_bins.detach().float().contiguous(),
                             va.energy_embedding.weight.detach().float().contiguous(), target=vals,
                             want_index=True)
    np.testing.assert_array_equal(idx.cpu().numpy()[0], g["index"])
    np.testing.assert_array_equal(x.cpu().numpy()[0], g["emb"])


@pytest.mark.parametrize("tag,max_len", [("none", None), ("given", 16), ("crop", 6)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_length_regulator_exact(tag, max_len, dt):
    from visual_onoma_to_wave_amd.model.modules import LengthRegulator
    g = golden("length_regulator")
    x = cuda(g["x"]).to(dt)
    out, mel_len = LengthRegulator()(x, cuda(g["d"]), max_len)
    np.testing.assert_array_equal(mel_len.cpu().numpy(), g["mel_len_" + tag])
    ref = torch.from_numpy(g["out_" + tag]).to(dt).float().numpy()  # bf16: same rounding as x
    np.testing.assert_array_equal(out.float().cpu().numpy(), ref)


def test_length_regulator_indices_vs_oracle_large():
    """C2-sized LR (B=32, T_src=12, D=256, 512 frames) + ragged/zero/fractional durations:
    frame -> token indices bit-exact against the oracle."""
    from oracle.acoustic import length_regulate
    from visual_onoma_to_wave_amd import ops
    rng = np.random.default_rng(5)
    d = rng.integers(0, 90, size=(32, 12)).astype(np.float32) + rng.choice([0, 0.5, 0.99], size=(32, 12))
    d[3] = 0
    d[7, ::2] = -1.0
    x = rng.normal(size=(32, 12, 256)).astype(np.float32)
    ref_out, ref_len, ref_idx = length_regulate(torch.from_numpy(x), d, 512)
    out, mel_len, idx = ops.length_regulate(cuda(x), cuda(d), 512, want_index=True)
    np.testing.assert_array_equal(mel_len.cpu().numpy(), ref_len.numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out.numpy())


def test_mask_exact():
    from visual_onoma_to_wave_amd.utils.tools import get_mask_from_lengths
    g = golden("mask")
    np.testing.assert_array_equal(get_mask_from_lengths(cuda(g["lens"])).cpu().numpy(), g["mask_none"])
    np.testing.assert_array_equal(get_mask_from_lengths(cuda(g["lens"]), 9).cpu().numpy(), g["mask_9"])
    np.testing.assert_array_equal(get_mask_from_lengths(cuda(g["lens"]).float(), 9).cpu().numpy(), g["mask_9"])


@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, BF16)])
def test_postnet(vtts, dt, tol):
    g = golden("postnet")
    vtts.postnet.set_compute_dtype(dt)
    with torch.no_grad():
        out = vtts.postnet(cuda(g["x"]))
    assert rel_l2(out.cpu(), g["out"]) < tol


# ------------------------------------------------------------------------------ whole acoustic model

NAMES = ["mel", "postnet_mel", "e_pred", "k_pred", "log_d_pred", "d_rounded",
         "src_masks", "mel_masks", "src_lens_out", "mel_lens_out"]


def _run_vtts(m, g, teacher):
    kw = {}
    if teacher:
        args = (cuda(g["in_audiotypes"]), cuda(g["in_texts"]), cuda(g["in_src_lens"]), int(g["in_max_src_len"]),
                cuda(g["in_mels"]), cuda(g["in_mel_lens"]), int(g["in_max_mel_len"]), cuda(g["in_e_targets"]),
                None, cuda(g["in_d_targets"]), cuda(g["in_images"]), None, True)
    else:
        args = (cuda(g["in_audiotypes"]), cuda(g["in_texts"]), cuda(g["in_src_lens"]), int(g["in_max_src_len"]),
                None, None, None, None, None, None, cuda(g["in_images"]), None, True)
        kw = dict(e_control=float(g["e_control"]), d_control=float(g["d_control"]))
    with torch.no_grad():
        return m(*args, **kw)


def _check(out, g, tol):
    for n, o in zip(NAMES, out):
        if o is None:
            assert n not in g, n
            continue
        o = o.cpu()
        if o.dtype in (torch.bool, torch.int64) or n == "d_rounded":
            np.testing.assert_array_equal(o.numpy(), g[n], err_msg=n)
        else:
            assert rel_l2(o, g[n]) < tol, (n, rel_l2(o, g[n]))


@pytest.mark.parametrize("mode,tol", [("fp32", F32_MODEL), ("mixed", BF16), ("bf16", 5e-2)])
def test_vtts_teacher_forced(vtts, mode, tol):
    _prec(vtts, mode)
    g = golden("vtts_tf")
    _check(_run_vtts(vtts, g, True), g, tol)


@pytest.mark.parametrize("tag", ["inf", "inf_ctrl"])
@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_vtts_inference(vtts, tag, mode):
    """Predicted energy bins and durations: d_rounded / mel_len / masks exact (the
    encoder and variance adaptor run fp32 in both modes)."""
    _prec(vtts, mode)
    g = golden("vtts_" + tag)
    b = vtts.variance_adaptor.duration_predictor.linear_layer.bias
    with torch.no_grad():
        b += float(g["dur_bias_shift"])
    try:
        _check(_run_vtts(vtts, g, False), g, F32_MODEL if mode == "fp32" else BF16)
    finally:
        with torch.no_grad():
            b -= float(g["dur_bias_shift"])


# ------------------------------------------------------------------------------ vocoder

@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, BF16)])
def test_resblocks(gen, stage, dt, tol):
    g = golden(f"resblock_s{stage}")
    for j, k in enumerate((3, 7, 11)):
        rb = gen.resblocks[3 * stage + j]
        rb.set_compute_dtype(dt)
        with torch.no_grad():
            out = rb(cuda(g["x"]))
        assert rel_l2(out.cpu(), g[f"k{k}"]) < tol, (stage, k)


@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, BF16)])
def test_upsamplers(gen, dt, tol):
    from visual_onoma_to_wave_amd import ops
    g = golden("ups")
    h = hifigan_h()
    gen.set_compute_dtype(dt)
    p = gen._packed(torch.device("cuda"), gen._build)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        w, b, cout, uu, pad = p["ups"][i]
        x = ops.transpose_bct(cuda(g[f"x{i}"]), dt)
        y = ops.conv1d(x, w, b, Co=u * cout, K=2, pad=1, pre_act=ops.ACT_LRELU, pre_slope=0.1,
                       transposed=dict(stride=u, pad=pad, cout=cout), out_dtype=torch.float32,
                       compute_dtype=dt)
        ref = g[f"y{i}"]
        assert y.shape == (1, ref.shape[2], ref.shape[1])
        assert rel_l2(y.cpu().numpy().transpose(0, 2, 1), ref) < tol, i


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_generator(gen, dt):
    """fp32 <= 1e-4; bf16 held to helpers.bf16_bar: max(1e-2, the reference's own bf16 autocast drift
    on these weights, 1.31e-2)."""
    import numpy as _np
    from helpers import bf16_bar, oracle_generator_bf16
    from oracle import vocoder as V
    g = golden("generator")
    gen.set_compute_dtype(dt)
    with torch.no_grad():
        wav = gen(cuda(g["mel"]))
    assert wav.shape == g["wav"].shape
    tol = F32_MODEL
    if dt == torch.bfloat16:
        gsd = V.fold_weight_norm({k: torch.from_numpy(_np.array(v)) for k, v in hifigan_arrays().items()})
        tol = bf16_bar(g["wav"], oracle_generator_bf16(gsd, torch.from_numpy(g["mel"]), hifigan_h()))
    assert rel_l2(wav.cpu(), g["wav"]) < tol


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_generator_bf16_reference_init(device, seed):
    """bf16 Generator on weights drawn the way the reference itself draws them: Generator(h) under
    weight_norm with PyTorch's default conv init (scripts/hifigan/models.py:10-13,58,94,146-147 --
    init_weights writes ``m.weight``, which the weight-norm hook recomputes from v and g at every
    forward, so v keeps the default init and g = ||v||), a C3-style mel clamp(N(-5, 2)) at
    B = 2 x 96 frames, against the fp32 oracle on the CPU.  Bar: no worse than the reference's own
    bf16 arithmetic on the same weights and mel -- this path's rel-L2 <= the CPU bf16 autocast's
    rel-L2 of the oracle Generator (the residual stream is bf16 in both: every stage input of the
    autocast run comes out of a bf16 conv), no slack; on seed 0 (the survey's measured case) also the
    survey's fixed 1e-2.  Per-stage local errors: tools/probes/gen_err_probe.py."""
    from visual_onoma_to_wave_amd import hifigan
    from helpers import oracle_generator_bf16
    from oracle import vocoder as V
    h = hifigan_h()
    torch.manual_seed(seed)
    g = hifigan.Generator(hifigan.AttrDict(h))
    sd = V.fold_weight_norm({k: v.detach().clone() for k, v in g.state_dict().items()})
    g.eval()
    g.remove_weight_norm()
    g = g.to(device)
    gen_cpu = torch.Generator().manual_seed(100 + seed)
    mel = torch.clamp(torch.randn(2, 80, 96, generator=gen_cpu) * 2.0 - 5.0, -11.513, 2.5)
    ref = V.generator(sd, mel, h)
    g.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        wav = g(mel.to(device)).float().cpu()
    assert wav.shape == ref.shape
    err = rel_l2(wav, ref)
    drift = rel_l2(oracle_generator_bf16(sd, mel, h), ref)
    print(f"seed {seed}: HIP bf16 rel-L2 {err:.3e}, reference bf16 autocast {drift:.3e}")
    assert err <= drift, (err, drift)
    if seed == 0:
        assert err < 1e-2, err


# ------------------------------------------------------------------------------ kernels vs oracle

@pytest.mark.parametrize("B,T,Ci,Co,K,dil,act", [
    (2, 300, 256, 256, 3, 1, 0), (3, 257, 128, 128, 7, 3, 2), (2, 1000, 64, 64, 11, 5, 2),
    (1, 777, 32, 32, 11, 5, 2), (4, 100, 256, 1024, 9, 1, 1), (2, 64, 1024, 256, 1, 1, 0),
    (2, 50, 80, 512, 7, 1, 0), (2, 33, 512, 80, 5, 1, 0), (1, 384, 2448, 256, 1, 1, 1),
    # short-sequence tiles (T_out <= 16 / <= 32: encoder / phoneme-level predictors)
    (32, 12, 256, 1024, 9, 1, 1), (5, 16, 1024, 256, 1, 1, 0), (3, 17, 256, 256, 3, 1, 1), (2, 32, 256, 192, 3, 1, 0),
    (3, 7, 256, 64, 9, 1, 1), (7, 1, 64, 512, 3, 1, 0), (6, 16, 32, 48, 5, 2, 2),
    # Co % 8 == 4: the lane's 8-channel run crosses the end of the output row
    (2, 40, 64, 20, 3, 1, 0), (3, 9, 32, 28, 5, 1, 2)])
@pytest.mark.parametrize("dt,tol", [(torch.float32, F32_MOD), (torch.bfloat16, 1e-2)])
def test_conv1d_vs_torch_fp32(B, T, Ci, Co, K, dil, act, dt, tol):
    """The implicit-GEMM conv against the plain PyTorch fp32 op (CPU) on the same data."""
    import torch.nn.functional as F
    from visual_onoma_to_wave_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, T, Ci, generator=g)
    w = torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    res = torch.randn(B, T, Co, generator=g)
    pad = dil * (K - 1) // 2
    xin = F.leaky_relu(x, 0.1) if act == 2 else x
    ref = F.conv1d(xin.transpose(1, 2), w, b, padding=pad, dilation=dil).transpose(1, 2)
    if act == 1:
        ref = F.relu(ref)
    ref = (ref + res) * 0.5
    wp = ops.pack_conv_weight(w.cuda(), dt)
    out = ops.conv1d(x.cuda().to(dt) if dt == torch.bfloat16 else x.cuda(), wp, b.cuda(), Co=Co, K=K, dil=dil,
                     pad=pad, pre_act=ops.ACT_LRELU if act == 2 else 0, pre_slope=0.1,
                     post_act=ops.ACT_RELU if act == 1 else 0, res1=res.cuda(), out_scale=0.5,
                     out_dtype=torch.float32, compute_dtype=dt)
    assert rel_l2(out.cpu(), ref) < tol


@pytest.mark.parametrize("cfg", [0, 5, 6])
@pytest.mark.parametrize("B,T,C,K,dil", [(2, 1000, 256, 11, 5), (3, 300, 256, 3, 1), (1, 1, 256, 7, 3),
                                         (2, 4096, 256, 7, 3), (2, 517, 128, 11, 1)])
def test_conv1d_mrf_stage0_tiles(B, T, C, K, dil, cfg):
    """MRF stage-0 conv (variant 1: 256 x 256 tile with LDS-DMA weights -- role-split staging for
    k >= 5, conv_cfg 5 forces it, 6 disables it: both shipped code paths at every k) with lrelu prologue,
    residual and accumulate epilogue, against PyTorch fp32 at ragged T and Co < tile."""
    import torch.nn.functional as F
    from visual_onoma_to_wave_amd import _lib, ops
    g = torch.Generator().manual_seed(T * 7 + K)
    x = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    w = torch.randn(C, C, K, generator=g) / (C * K) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    res = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    pad = dil * (K - 1) // 2
    ref = F.conv1d(F.leaky_relu(x.float(), 0.1).transpose(1, 2), w, b, padding=pad, dilation=dil).transpose(1, 2)
    ref = (ref + res.float()) * 0.5
    wp = ops.pack_conv_weight(w.cuda(), torch.bfloat16)
    _lib.lib().vo_tune(b"conv_cfg", cfg)
    try:
        out = ops.conv1d(x.cuda(), wp, b.cuda(), Co=C, K=K, dil=dil, pad=pad, pre_act=ops.ACT_LRELU, pre_slope=0.1,
                         res1=res.cuda(), out_scale=0.5, variant=1)
        torch.cuda.synchronize()
    finally:
        _lib.lib().vo_tune(b"conv_cfg", 0)
    assert rel_l2(out.float().cpu(), ref) < 1e-2


@pytest.mark.parametrize("B,T,K,dil", [(2, 1000, 11, 5), (3, 300, 3, 1), (1, 1, 7, 3), (2, 4099, 7, 3)])
def test_conv1d_stage0_role_split_bit_identical(B, T, K, dil):
    """The role-split stage-0 conv (conv_cfg 5) equals the single-role kernel (conv_cfg 6) bit for bit,
    with both the residual and the MRF accumulator operands, at ragged T (tile edges, T = 1)."""
    from visual_onoma_to_wave_amd import _lib, ops
    C = 256
    g = torch.Generator().manual_seed(T + K)
    x = torch.randn(B, T, C, generator=g).to(torch.bfloat16).cuda()
    wp = ops.pack_conv_weight((torch.randn(C, C, K, generator=g) / (C * K) ** 0.5).cuda(), torch.bfloat16)
    b = (torch.randn(C, generator=g) * 0.1).cuda()
    res = torch.randn(B, T, C, generator=g).to(torch.bfloat16).cuda()
    acc = torch.randn(B, T, C, generator=g).to(torch.bfloat16).cuda()
    outs = []
    for cfg in (5, 6):
        _lib.lib().vo_tune(b"conv_cfg", cfg)
        try:
            outs.append(ops.conv1d(x, wp, b, Co=C, K=K, dil=dil, pad=dil * (K - 1) // 2, pre_act=ops.ACT_LRELU,
                                   pre_slope=0.1, res1=res, res2=acc, out_scale=1 / 3, variant=1))
            torch.cuda.synchronize()
        finally:
            _lib.lib().vo_tune(b"conv_cfg", 0)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("B,L,lens", [(4, 512, [512, 300, 1, 77]), (2, 1000, [1000, 999]), (3, 12, [12, 7, 5]),
                                      (2, 64, [64, 63]), (2, 65, [65, 1]), (1, 1, [1]), (2, 129, [100, 129])])
@pytest.mark.parametrize("dt,tol,cfg", [(torch.float32, F32_MOD, 0), (torch.bfloat16, 1e-2, 0),
                                        (torch.bfloat16, 1e-2, 1)])
def test_attention_vs_oracle(B, L, lens, dt, tol, cfg):
    """vo_attention vs the PyTorch fp32 SDPA with key padding; bf16 for both kernels (att_cfg 0 =
    the S^T / register-P kernel, 1 = the first version)."""
    from visual_onoma_to_wave_amd import _lib, ops
    _lib.lib().vo_tune(b"att_cfg", cfg)
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(B, L, 768, generator=g)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    q, k, v = qkv.split(256, dim=-1)
    ref = torch.zeros(B, L, 256)
    for h in range(2):
        s = q[..., h * 128:(h + 1) * 128] @ k[..., h * 128:(h + 1) * 128].transpose(1, 2) / 128 ** 0.5
        s = s.masked_fill(torch.arange(L)[None, None, :] >= lens_t[:, None, None], -float("inf"))
        ref[..., h * 128:(h + 1) * 128] = torch.softmax(s, -1) @ v[..., h * 128:(h + 1) * 128]
    try:
        out = ops.attention(qkv.cuda().to(dt), lens_t.cuda(), 2)
        torch.cuda.synchronize()
    finally:
        _lib.lib().vo_tune(b"att_cfg", 0)
    assert rel_l2(out.float().cpu(), ref) < tol


# Tile edges are asked of the library when a test runs (vo_resblock3_tile_rows / vo_resblock_pair_tile_rows), so they
# follow a retiling: a length is an int, or m BT + add with BT the output rows per tile of the kernel that the
# dispatch picks for the named shape under the named knob value.  Each such case keeps the id of today's length.
def _r3(C, m=1, add=0, cfg=0, dils=(1, 3, 5)):
    return ("rb3_cfg", cfg, lambda ops: ops.resblock3_tile_rows(C, dils), m, add)


def _pr(C, k, d, m=1, add=0, cfg=0):
    return ("pair_cfg", cfg, lambda ops: ops.resblock_pair_tile_rows(C, k, d), m, add)


def _length(T):
    if isinstance(T, int):
        return T
    from visual_onoma_to_wave_amd import _lib, ops
    knob, cfg, query, m, add = T
    _lib.lib().vo_tune(knob.encode(), cfg)
    try:
        bt = query(ops)
    finally:
        _lib.lib().vo_tune(knob.encode(), 0)
    assert bt > 0
    return m * bt + add


def _resblock3_case(C, T, with_acc, cfg, dils):
    """vo_resblock3 under rb3_cfg `cfg` against the torch fp32 ResBlock, and against three vo_resblock_pair
    launches (same bf16 intermediates up to summation order)."""
    import torch.nn.functional as F
    from visual_onoma_to_wave_amd import ops
    T = _length(T)
    g = torch.Generator().manual_seed(C * 7 + T)
    B, k = 2, 3
    x = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    w1 = [torch.randn(C, C, k, generator=g) / (C * k) ** 0.5 for _ in dils]
    w2 = [torch.randn(C, C, k, generator=g) / (C * k) ** 0.5 for _ in dils]
    b1 = [torch.randn(C, generator=g) * 0.1 for _ in dils]
    b2 = [torch.randn(C, generator=g) * 0.1 for _ in dils]
    acc = torch.randn(B, T, C, generator=g).to(torch.bfloat16) if with_acc else None
    cur = x.float().transpose(1, 2)
    for s, d in enumerate(dils):
        t = F.leaky_relu(F.conv1d(F.leaky_relu(cur, 0.1), w1[s], b1[s], padding=d, dilation=d), 0.1)
        cur = F.conv1d(t, w2[s], b2[s], padding=1) + cur
    ref = (cur / 3.0).transpose(1, 2) + (acc.float() if with_acc else 0.0)
    p1 = [ops.pack_conv_weight(w.cuda(), torch.bfloat16) for w in w1]
    p2 = [ops.pack_conv_weight(w.cuda(), torch.bfloat16) for w in w2]
    b1c, b2c = [b.cuda() for b in b1], [b.cuda() for b in b2]
    xc = x.cuda()
    out = acc.cuda().clone() if with_acc else torch.empty_like(xc)
    from visual_onoma_to_wave_amd import _lib
    _lib.lib().vo_tune(b"rb3_cfg", cfg)  # every rb3_cfg kernel configuration (0 = shipped)
    try:
        ops.resblock3(xc, p1, b1c, p2, b2c, dils, 0.1, out=out, out_scale=1.0 / 3, acc=out if with_acc else None)
    finally:
        _lib.lib().vo_tune(b"rb3_cfg", 0)
    chain = xc
    for s, d in enumerate(dils):  # the per-pair path
        if s < 2:
            chain = ops.resblock_pair(chain, p1[s], b1c[s], p2[s], b2c[s], k, d, 0.1)
        else:
            o = acc.cuda().clone() if with_acc else torch.empty_like(xc)
            chain = ops.resblock_pair(chain, p1[s], b1c[s], p2[s], b2c[s], k, d, 0.1, out=o, out_scale=1.0 / 3,
                                      acc=o if with_acc else None)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out.float().cpu(), ref) < 1e-2
    assert rel_l2(out.float().cpu(), chain.float().cpu()) < 3e-3


@pytest.mark.parametrize("C,T", [(32, 1000), (64, 777), (128, 300), (32, 5), (64, 1), (128, 13),
                                 # edges of earlier tilings (232-row frames at C = 128, 488-row ones at C = 32): interior
                                 # lengths of today's kernels
                                 (128, 232), (128, 233), (32, 488 * 3 + 7),
                                 (64, 131072), (32, 65536), (128, 32768),
                                 # register-resident frames at C = 32 (today 104 output rows per tile): BT, BT + 1
                                 pytest.param(32, _r3(32), id="32-104"), pytest.param(32, _r3(32, 1, 1), id="32-105"),
                                 (32, 24),
                                 # the 72-row edges of the C = 64 register frames, a kernel since deleted:
                                 # interior lengths of the shipped plane kernel
                                 (64, 72), (64, 73), (64, 16), (64, 72 * 5 - 1),
                                 # wave-owned planes (resblock_pb3.hip; today 200 (C = 128) / 488 (C = 64) output rows
                                 # per tile): BT, BT + 1, 4 BT + 3 / 3 BT + 5
                                 pytest.param(128, _r3(128), id="128-200"), pytest.param(128, _r3(128, 1, 1), id="128-201"),
                                 pytest.param(128, _r3(128, 4, 3), id="128-803"),
                                 pytest.param(64, _r3(64), id="64-488"), pytest.param(64, _r3(64, 1, 1), id="64-489"),
                                 pytest.param(64, _r3(64, 3, 5), id="64-1469"),
                                 # the C = 32 LDS-frame kernel's own edge (rb3_cfg 80; today 256-row frames, 232 output
                                 # rows per tile): BT, BT + 1
                                 pytest.param(32, _r3(32, cfg=80), id="32-232"),
                                 pytest.param(32, _r3(32, 1, 1, cfg=80), id="32-233")])
@pytest.mark.parametrize("with_acc", [True, False])
# cfg 0: the shipped dispatch (C = 32: register-resident frames; C = 64 / 128: wave-owned planes).  80 (any
# rb3_cfg != 0): the LDS-frame kernel at C = 32; at C = 64 / 128 the library has the plane kernel alone and runs it
# whatever the knob says
@pytest.mark.parametrize("cfg", [0, 80])
def test_fused_resblock3_vs_torch_fp32(C, T, with_acc, cfg):
    """vo_resblock3 (a whole k = 3 ResBlock, dilations 1/3/5, in one launch) against the torch fp32
    ResBlock at tile edges (asked of the library), T = 1, and multi-tile persistent runs;
    and against three vo_resblock_pair launches (same bf16 intermediates up to summation order)."""
    _resblock3_case(C, T, with_acc, cfg, (1, 3, 5))


@pytest.mark.parametrize("with_acc", [True, False])
@pytest.mark.parametrize("T", [1, pytest.param(_r3(32, dils=(1, 2, 4)), id="232"),
                               pytest.param(_r3(32, 1, 1, dils=(1, 2, 4)), id="233"),
                               pytest.param(_r3(32, 3, 7, dils=(1, 2, 4)), id="703")])
def test_fused_resblock3_c32_lds_frames_by_default(T, with_acc):
    """C = 32 off the (1, 3, 5) fast path: dilations (1, 2, 4) (halo 10 <= 12) run the LDS-frame kernel with no knob
    set -- the only shipped code for them -- at its tile edges BT, BT + 1 and 3 BT + 7 (today 232 output rows per
    256-row frame)."""
    _resblock3_case(32, T, with_acc, 0, (1, 2, 4))


# cfg 0: the shipped dispatch (wave-owned planes for C = 64 / 128 k = 7 / 11); 93 and, at C = 64, 111: the LDS-tile
# kernels there too, the generic ones that also serve k = 5 / 9 / 13 / 15
_PAIR_CFGS = [0, 93, 111]


def _pair_case(C, T, k, d, with_acc, cfg):
    """vo_resblock_pair under pair_cfg `cfg` against torch fp32."""
    import torch.nn.functional as F
    from visual_onoma_to_wave_amd import _lib, ops
    T = _length(T)
    g = torch.Generator().manual_seed(C * T + k)
    B = 2
    x = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    w1 = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    w2 = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    acc = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    xf = x.float().transpose(1, 2)
    t = F.leaky_relu(F.conv1d(F.leaky_relu(xf, 0.1), w1, b1, padding=d * (k - 1) // 2, dilation=d), 0.1)
    scale = 1.0 / 3 if with_acc else 1.0
    ref = ((F.conv1d(t, w2, b2, padding=(k - 1) // 2) + xf) * scale).transpose(1, 2)
    if with_acc:
        ref = ref + acc.float()
    p1 = ops.pack_conv_weight(w1.cuda(), torch.bfloat16)
    p2 = ops.pack_conv_weight(w2.cuda(), torch.bfloat16)
    out = acc.cuda().clone() if with_acc else torch.full_like(x.cuda(), float("nan"))
    _lib.lib().vo_tune(b"pair_cfg", cfg)
    try:
        ops.resblock_pair(x.cuda(), p1, b1.cuda(), p2, b2.cuda(), k, d, 0.1, out=out, out_scale=scale,
                          acc=out if with_acc else None)
        torch.cuda.synchronize()
    finally:
        _lib.lib().vo_tune(b"pair_cfg", 0)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out.float().cpu(), ref) < 1e-2


@pytest.mark.parametrize("cfg", _PAIR_CFGS)
@pytest.mark.parametrize("with_acc", [True, False])
@pytest.mark.parametrize("C,T,k,d", [(32, 1000, 11, 5), (64, 777, 7, 3), (32, 5, 3, 1), (64, 1, 11, 1),
                                     # (3 x 246: three tiles of an earlier C = 32 tiling; an interior length today)
                                     (32, 246 * 3, 11, 5), (64, 4096, 3, 5),
                                     pytest.param(64, _pr(64, 11, 3), 11, 3, id="64-502-11-3"),
                                     # several tiles per persistent workgroup (pipelined window/weights)
                                     (32, 131072, 11, 5), (32, 65536, 3, 1), (64, 65536, 7, 3),
                                     (64, 65536, 3, 1), (64, 40000, 11, 5),
                                     # C = 64 k = 7 / 11 plane kernel: one tile (today 502 / 506 valid rows), + 1,
                                     # two + 1
                                     pytest.param(64, _pr(64, 11, 5, 1, 1), 11, 5, id="64-503-11-5"), (64, 13, 7, 1),
                                     pytest.param(64, _pr(64, 7, 5, 2, 1), 7, 5, id="64-1013-7-5"),
                                     pytest.param(64, _pr(64, 7, 3), 7, 3, id="64-506-7-3"),
                                     (128, 300, 3, 1), (128, 20000, 3, 5),
                                     # C = 128 k = 7 / 11: T = 1, one tile, tile edges (today 246 / 250 valid
                                     # rows: BT, BT + 1, BT, 2 BT + 1), utterances crossing inside a workgroup's
                                     # run, every dilation
                                     (128, 1, 7, 3), (128, 1, 11, 5), (128, 13, 11, 1),
                                     pytest.param(128, _pr(128, 11, 5), 11, 5, id="128-246-11-5"),
                                     pytest.param(128, _pr(128, 11, 3, 1, 1), 11, 3, id="128-247-11-3"),
                                     pytest.param(128, _pr(128, 7, 1), 7, 1, id="128-250-7-1"),
                                     pytest.param(128, _pr(128, 7, 5, 2, 1), 7, 5, id="128-501-7-5"),
                                     (128, 5000, 11, 3),
                                     (128, 32768, 11, 5), (128, 32768, 7, 3), (128, 20011, 11, 1)])
def test_fused_resblock_pair_vs_torch_fp32(C, T, k, d, with_acc, cfg):
    """vo_resblock_pair (c1 -> lrelu -> c2 + residual, MRF accumulate) at tile edges vs torch fp32,
    for the shipped dispatch and the LDS-tile kernels behind pair_cfg 93 / 111."""
    _pair_case(C, T, k, d, with_acc, cfg)


@pytest.mark.parametrize("with_acc", [True, False])
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("edge", ["one", "bt", "bt+1", "2bt+3"])
@pytest.mark.parametrize("k", [5, 9])
@pytest.mark.parametrize("C", [64, 128])
def test_fused_resblock_pair_generic_k(C, k, edge, d, with_acc):
    """k = 5 / 9 at C = 64 / 128: shapes only the generic LDS-tile kernels serve (no knob set), at T = 1, one full
    tile, one row more, and two tiles and three rows (the tile's rows asked of the library)."""
    from visual_onoma_to_wave_amd import ops
    bt = ops.resblock_pair_tile_rows(C, k, d)
    assert bt > 0
    T = {"one": 1, "bt": bt, "bt+1": bt + 1, "2bt+3": 2 * bt + 3}[edge]
    _pair_case(C, T, k, d, with_acc, 0)


@pytest.mark.parametrize("with_acc,scale", [(True, 1.0 / 3), (False, 1.0), (True, 0.3)])
@pytest.mark.parametrize("T,k,d", [(32768, 11, 5), (20011, 7, 3), (777, 11, 1), (1, 7, 5),
                                   # one tile of the C = 128 kernel (today 250 rows)
                                   pytest.param(_pr(128, 7, 1), 7, 1, id="250-7-1")])
@pytest.mark.parametrize("C", [128, 64])
def test_pair_plane_frag_bit_identical(C, T, k, d, with_acc, scale):
    """vo_resblock_pair_frag (weights in the fragment order of vo_pack_frag, each load one contiguous
    KiB) equals the plane kernel on the [K][Co][Ci] packs bit for bit (vo_resblock_pair): same kernel,
    same summation order; out_scale 0.3 takes the epilogue-add path for the MRF accumulator (1 / 0.3 is
    not a bf16 value)."""
    from visual_onoma_to_wave_amd import ops
    B = 3
    T = _length(T)
    g = torch.Generator(device="cuda").manual_seed(T + 10 * k + d)
    x = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16)
    acc = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16)
    p1 = ops.pack_conv_weight(torch.randn(C, C, k, device="cuda", generator=g) / (C * k) ** 0.5, torch.bfloat16)
    p2 = ops.pack_conv_weight(torch.randn(C, C, k, device="cuda", generator=g) / (C * k) ** 0.5, torch.bfloat16)
    b1 = torch.randn(C, device="cuda", generator=g) * 0.1
    b2 = torch.randn(C, device="cuda", generator=g) * 0.1
    outs = []
    for frag in (False, True):
        w1, w2 = (ops.pack_frag(p1), ops.pack_frag(p2)) if frag else (p1, p2)
        o = acc.clone()
        ops.resblock_pair(x, w1, b1, w2, b2, k, d, 0.1, out=o, out_scale=scale, acc=o if with_acc else None,
                          frag=frag)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    # and against torch fp32 (the accumulator path with its epilogue add or identity MFMA)
    import torch.nn.functional as F
    if T <= 1000:
        w1f = p1.float().permute(1, 2, 0)  # [K][Co][Ci] -> (Co, Ci, K)
        w2f = p2.float().permute(1, 2, 0)
        xf = x.float().transpose(1, 2)
        t = F.leaky_relu(F.conv1d(F.leaky_relu(xf, 0.1), w1f, b1, padding=d * (k - 1) // 2, dilation=d), 0.1)
        ref = ((F.conv1d(t, w2f, b2, padding=(k - 1) // 2) + xf) * scale).transpose(1, 2)
        if with_acc:
            ref = ref + acc.float()
        assert rel_l2(outs[1].float().cpu(), ref.cpu()) < 1e-2


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", [256, 512])
def test_layernorm_dual_bf16_copy(D, dt):
    """vo_layernorm_dual: y bit-identical to vo_layernorm's fp32 y, y16 exactly y rounded to bf16
    (nearest even) -- what a bf16 conv's staging makes of y -- pad rows 0 in both."""
    from visual_onoma_to_wave_amd import ops
    g = torch.Generator(device="cuda").manual_seed(D)
    xdt = torch.float32 if dt == "f32" else torch.bfloat16
    B, T = 3, 77
    x = torch.randn(B, T, D, device="cuda", generator=g).to(xdt)
    res = torch.randn(B, T, D, device="cuda", generator=g).to(xdt)
    gam = torch.randn(D, device="cuda", generator=g)
    bet = torch.randn(D, device="cuda", generator=g)
    lens = torch.tensor([77, 40, 1], dtype=torch.int32, device="cuda")
    y1 = ops.layernorm(x, gam, bet, res=res, lens=lens, out_dtype=torch.float32)
    y, y16 = ops.layernorm(x, gam, bet, res=res, lens=lens, out_dtype=torch.float32, with_bf16=True)
    torch.cuda.synchronize()
    assert torch.equal(y, y1)
    assert torch.equal(y16, y.to(torch.bfloat16))
    assert not y16[1, 40:].any() and not y16[2, 1:].any()


def test_decoder_ln_bf16_copy_bit_identical(vtts):
    """The mixed decoder with the LayerNorms' bf16 copies feeding the q/k/v and FFN w_1 convs
    (vo_layernorm_dual) gives bit-for-bit the outputs of converting the fp32 stream in the convs."""
    from visual_onoma_to_wave_amd.transformer.Models import Decoder
    _prec(vtts, "mixed")
    g = golden("vtts_tf")
    outs = []
    for flag in (False, True):
        Decoder.ln_bf16_copy = flag
        try:
            outs.append(_run_vtts(vtts, g, True))
        finally:
            Decoder.ln_bf16_copy = True
    for a, b in zip(outs[0], outs[1]):
        if torch.is_tensor(a):
            assert torch.equal(a, b)
