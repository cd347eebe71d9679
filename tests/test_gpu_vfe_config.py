"""The glyph encoder's config surface on the GPU: vo_vfe_stencil_ex (context stride, kh x kw taps, any depth)
per element and per tensor against the float64 yardstick of tests/vfe_check.py, its guards and its LDS bound;
VisualFeatureExtractor and vTTS against goldens recorded from the reference at those configurations; the
training conv (vo_vfe_conv_*_ex) and the module's training path against float64 autograd.

Bars: one layer per element |got - ref| <= 2 (R + 8) 2^-24 A (tests/conv_check.py's form, R = kh kw,
A = (conv(|x|, |w|) + |b|) |scale| + |shift|), bf16 output + 2^-8 |ref|; stacks rel-L2 < 1e-5
(conv_check.REL_L2_F32), bf16 output after 2^-8 |ref| is taken off every element's error; modules 2e-5 / 1e-2 and the whole model 1e-4 / 1e-2
(test_gpu_parity's F32_MOD, BF16, F32_MODEL); training 1e-5 (test_gpu_train_glue.test_vfe_conv_fwd_bwd's)."""

import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_check as CC
import test_gpu_parity as P
import vfe_check as V
from helpers import configs, golden, rel_l2, spec
from weights import load_into, make_state_dict

pytestmark = pytest.mark.gpu

GUARD_ROWS = 2


def _guarded(rows, cols, dt, device):
    """(buffer, view): the (rows, cols) output view with GUARD_ROWS rows of conv_check.Y_GUARD before and after."""
    buf = torch.empty((rows + 2 * GUARD_ROWS, cols), dtype=dt, device=device)
    buf.view(CC._INT[dt]).fill_(CC.Y_GUARD[dt])
    return buf, buf[GUARD_ROWS:GUARD_ROWS + rows]


def _guards_intact(buf, rows):
    raw = buf.view(CC._INT[buf.dtype])
    return bool((raw[:GUARD_ROWS] == CC.Y_GUARD[buf.dtype]).all()) and \
        bool((raw[GUARD_ROWS + rows:] == CC.Y_GUARD[buf.dtype]).all())


def _run(c, dt, device):
    """The case through ops.vfe_stencil_ex into a guarded view -> (result on the CPU, guards intact)."""
    from visual_onoma_to_wave_amd import ops
    kh, kw = c["kernel"]
    rows, cols = c["images"].shape[0] * c["n"], c["H"] * c["slice_w"] * c["stride"]
    buf, view = _guarded(rows, cols, dt, device)
    out, n = ops.vfe_stencil_ex(c["images"].to(device), c["conv"].to(device), c["bn"].to(device), c["slice_w"],
                                c["stride"], (kh, kw), dt, out=view)
    torch.cuda.synchronize()
    assert n == c["n"] and out.data_ptr() == view.data_ptr()
    return view.cpu(), _guards_intact(buf, rows)


@functools.lru_cache(maxsize=None)
def _case(shape, layers):
    c = V.shape_case(shape, layers)
    ref, bar, alive = V.stencil64(c)
    assert alive >= V.ALIVE_MIN, (c["name"], alive)
    return c, ref, bar


# ------------------------------------------------------------------------------------ 1. the ICASSP point

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_ex_equals_icassp_stencil_bit_for_bit(device, dt):
    from visual_onoma_to_wave_amd import ops
    c = V.stencil_case(2024, 2, 24, 102, 1, 3, 3, 3, 3)
    img, conv, bn = c["images"].to(device), c["conv"].to(device), c["bn"].to(device)
    old, n_old = ops.vfe_stencil(img, conv, bn, 102, dt)
    new, n_new = ops.vfe_stencil_ex(img, conv, bn, 102, 1, (3, 3), dt)
    assert n_old == n_new == 3 and old.shape == new.shape == (6, 24 * 102) and new.dtype == dt
    assert float((old.float() != 0).float().mean()) >= V.ALIVE_MIN
    assert torch.equal(old, new)


# ------------------------------------------------------------------------------------ 2. one layer, per element

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_single_layer_per_element(device, shape, dt):
    c, ref, bar = _case(shape, 1)
    got, intact = _run(c, dt, device)
    got = got.double()
    if dt == torch.bfloat16:
        bar = bar + 2.0 ** -8 * ref.abs()
    err = (got - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    print(f"{c['name']} {dt}: worst error / bar {ratio:.3e}, rel-L2 {rel_l2(got, ref):.3e}")
    assert bool(torch.isfinite(got).all())
    over = err > bar
    assert not bool(over.any()), f"{int(over.sum())} of {over.numel()} over the bar (worst {ratio:.3g}), first at " \
                                 f"{tuple(int(i) for i in over.nonzero()[0])}"
    assert intact, "guard rows written"


# ------------------------------------------------------------------------------------ 3. stacks (+ 4. guards)

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_layer_stacks(device, shape, dt):
    for layers in V.DEPTHS:
        c, ref, _ = _case(shape, layers)
        got, intact = _run(c, dt, device)
        err = (got.double() - ref).abs()
        if dt == torch.bfloat16:  # per element 2^-8 |ref| for the output's rounding; what exceeds it meets the fp32 bar
            err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
        e = float(err.norm() / ref.norm())
        print(f"{c['name']} {dt}: rel-L2 {e:.3e}" + (" beyond 2^-8 |ref|" if dt == torch.bfloat16 else ""))
        assert bool(torch.isfinite(got).all())
        assert e < CC.REL_L2_F32, (c["name"], e)
        assert intact, (c["name"], "guard rows written")


# ------------------------------------------------------------------------------------ 5. the LDS boundary

def test_lds_boundary(device):
    from visual_onoma_to_wave_amd import _lib, ops
    H, bound = 24, 160 * 1024
    w = 1
    while ops.vfe_stencil_lds_bytes(H, w + 1, 3, 3) <= bound:
        w += 1
    assert ops.vfe_stencil_lds_bytes(H, w, 3, 3) <= bound < ops.vfe_stencil_lds_bytes(H, w + 1, 3, 3) and w > 510
    # the widest window the query accepts: one window, W = win_w
    c = V.stencil_case(77, 1, H, w, 1, 1, 3, 3, 3)
    ref, _, alive = V.stencil64(c)
    assert alive >= V.ALIVE_MIN
    got, intact = _run(c, torch.float32, device)
    e = rel_l2(got.double(), ref)
    print(f"H {H}, win_w {w} ({ops.vfe_stencil_lds_bytes(H, w, 3, 3)} B): rel-L2 {e:.3e}")
    assert e < CC.REL_L2_F32 and intact
    # one column wider: an error return through _lib.check, nothing written
    c = V.stencil_case(78, 1, H, w + 1, 1, 1, 3, 3, 1)
    buf, view = _guarded(1, H * (w + 1), torch.float32, device)
    with pytest.raises(RuntimeError, match="160 KiB"):
        ops.vfe_stencil_ex(c["images"].to(device), c["conv"].to(device), c["bn"].to(device), w + 1, 1, (3, 3),
                           torch.float32, out=view)
    torch.cuda.synchronize()
    raw = buf.view(torch.int32)
    assert bool((raw == CC.Y_GUARD[torch.float32]).all()), "a refused call wrote its output"
    assert isinstance(_lib.lib().vo_last_error(), bytes)


# ------------------------------------------------------------------------------------ 6. module goldens

@pytest.mark.parametrize("dt,tol", [(torch.float32, P.F32_MOD), (torch.bfloat16, P.BF16)], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", V.GOLDEN_CASES)
def test_module_goldens(device, name, dt, tol):
    g = golden("vfe_cfg_" + name)
    cfg, sd = V.golden_config(g)
    m = V.build_module(cfg, 10, 8, 32)
    load_into(m, sd)
    m = m.to(device).eval().set_compute_dtype(dt)
    with torch.no_grad():
        out = m(P.cuda(g["images"]))
    e = rel_l2(out.float().cpu(), g["out"])
    print(f"vfe_cfg_{name} {dt}: rel-L2 {e:.3e}")
    assert out.shape == g["out"].shape and e < tol


# ------------------------------------------------------------------------------------ 7. the whole model

def _configs_s3():
    pc, mc, tc = configs()
    pc = copy.deepcopy(pc)
    pc["visual_text"]["stride"] = 3
    return pc, mc, tc


@pytest.fixture(scope="module")
def vtts_s3(device):
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*_configs_s3())
    seed, sp = spec("vtts_s3")
    load_into(m, make_state_dict(sp, seed))
    return m.to(device).eval()


def _padded_inputs():
    """vtts_tf's inputs, the images with pad_2D_gray_image's stride-3 margins: 102 white columns on each side."""
    g = dict(golden("vtts_tf"))
    g["in_images"] = np.pad(g["in_images"], [(0, 0), (0, 0), (0, 0), (102, 102)], mode="constant", constant_values=1.0)
    return g


@pytest.mark.parametrize("mode,tol", [("fp32", P.F32_MODEL), ("mixed", P.BF16)])
def test_vtts_teacher_forced_stride3(vtts_s3, mode, tol):
    P._prec(vtts_s3, mode)
    ref = golden("vtts_tf_s3")
    out = P._run_vtts(vtts_s3, _padded_inputs(), True)
    print(f"vtts_tf_s3 {mode}: mel {rel_l2(out[0].cpu(), ref['mel']):.3e}, postnet_mel "
          f"{rel_l2(out[1].cpu(), ref['postnet_mel']):.3e}")
    P._check(out, ref, tol)
    # stride 3 is another function of the same strip: the stride-1 golden is far away
    assert rel_l2(ref["postnet_mel"], golden("vtts_tf")["postnet_mel"]) > 100 * P.F32_MODEL


def test_glyph_batch_stride3_through_encoder(vtts_s3, device):
    """dataset.GlyphBatch lays out the stride-3 margins, and the encoder cuts exactly max_src_len windows."""
    from visual_onoma_to_wave_amd.dataset import GlyphBatch
    rng = np.random.default_rng(5)
    widths = [rng.integers(20, 103, size=n) for n in (6, 4)]
    strips = [rng.integers(0, 256, size=(24, int(w.sum())), dtype=np.uint8) for w in widths]
    images = GlyphBatch(strips, widths, 102, 3).to(device)
    assert tuple(images.shape) == (2, 1, 24, 102 * (6 + 2))
    assert bool((images[..., :102] == 1).all()) and bool((images[..., -102:] == 1).all())
    P._prec(vtts_s3, "fp32")
    src = torch.ones(2, 6, dtype=torch.long, device=device)
    lens = torch.tensor([6, 4], dtype=torch.int32, device=device)
    with torch.no_grad():
        x = vtts_s3.encoder.run(src, lens, images)
        emb = vtts_s3.encoder.VisualFeatureExtractor(images)
    assert tuple(x.shape) == (2, 6, 256) and tuple(emb.shape) == (2, 6, 256) and bool(torch.isfinite(x).all())
    sd = {k.split("VisualFeatureExtractor.")[1]: v.detach().double().cpu()
          for k, v in vtts_s3.state_dict().items() if "VisualFeatureExtractor." in k}
    ref = V.extractor64(sd, images.double().cpu(), slice_w=102, stride=3, kernel=(3, 3), layers=3, norm=True, relu=True)
    assert rel_l2(emb.cpu(), ref) < P.F32_MOD


# ------------------------------------------------------------------------------------ 8. the training conv

def _conv64(N, H, W, kh, kw):
    g = torch.Generator().manual_seed(N * H + W + 100 * kh + kw)
    w = torch.rand(1, 1, kh, kw, generator=g) - 0.5
    b = torch.rand(1, generator=g) * 0.2 - 0.1
    x = torch.rand(N, 1, H, W, generator=g, dtype=torch.float64)
    gy = torch.randn(N, 1, H, W, generator=g, dtype=torch.float64)
    xr, wr, br = x.clone().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, padding=((kh - 1) // 2, (kw - 1) // 2))
    (yr * gy).sum().backward()
    return x, gy, w, b, dict(y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)


def _check_conv(tag, got, ref):
    errs = {k: rel_l2(got[k].cpu(), ref[k]) for k in ref}
    print(tag, {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 1e-5 for v in errs.values()), errs


def test_vfe_conv_ex_entries_directly(device):
    """(N, H, W) = (1, 1, 1) under a 3 x 3 kernel through vo_vfe_conv_fwd_ex / vo_vfe_conv_bwd_ex themselves
    (autograd.vfe_conv sends 3 x 3 to the ICASSP entries)."""
    from visual_onoma_to_wave_amd import ops
    x, gy, w, b, ref = _conv64(1, 1, 1, 3, 3)
    wv = torch.cat([w.reshape(-1), b]).to(device)
    xg, gg = x.float().to(device), gy.float().to(device)
    y = ops.vfe_conv_fwd_ex(xg, wv, 3, 3)
    dx, dw = ops.vfe_conv_bwd_ex(xg, gg, wv, 3, 3)
    _check_conv("(1, 1, 1, 3, 3)", dict(y=y, dx=dx, dw=dw[:9].view(1, 1, 3, 3), db=dw[9:]), ref)


@pytest.mark.parametrize("N,H,W,kh,kw", [(3, 5, 4, 5, 3), (2, 3, 4, 7, 9), (36, 24, 306, 3, 5)])
def test_vfe_conv_fwd_bwd(device, N, H, W, kh, kw):
    from visual_onoma_to_wave_amd import autograd as AG
    x, gy, w, b, ref = _conv64(N, H, W, kh, kw)
    conv = torch.nn.Conv2d(1, 1, (kh, kw), padding=((kh - 1) // 2, (kw - 1) // 2))
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    conv = conv.to(device)
    grads = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xg = x.float().to(device).requires_grad_(True)
        y = AG.vfe_conv(xg, conv)
        y.backward(gy.float().to(device))
        grads.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
    _check_conv((N, H, W, kh, kw), dict(y=y.detach(), dx=xg.grad, dw=conv.weight.grad, db=conv.bias.grad), ref)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), "dw is not reproducible"


# ------------------------------------------------------------------------------------ 9. the training module

@pytest.mark.parametrize("norm,relu", [(True, True), (False, False)], ids=["bn-relu", "plain"])
def test_train_run_vs_float64_autograd(device, norm, relu):
    """train_run + backward of a stride-3, [3, 5], 2-layer module (H = 8, slice_w = 10, embed 32, B = 2, 5
    characters, fp32) against float64 autograd of the yardstick with batch-statistics BatchNorm: the output and
    every parameter gradient rel-L2 < 1e-5 of its own norm, the running statistics within 1e-6.  One kind of
    gradient has no error relative to its own norm: a conv bias under BatchNorm is exactly zero (asserted of the
    float64 result) and is held to 1e-5 of the same conv's weight gradient."""
    cfg = dict(stride=3, kernel=(3, 5), layers=2, norm=norm, relu=relu)
    g = torch.Generator().manual_seed(31 + norm)
    m = V.build_module(cfg, 10, 8, 32)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            leaf = k.rsplit(".", 1)[1]
            if v.dim() == 4:
                v.copy_(torch.rand(v.shape, generator=g) - 0.5)
            elif k.startswith("embedder.") and leaf in ("weight", "running_var"):
                v.copy_(0.7 + 0.6 * torch.rand(v.shape, generator=g))
            elif k.startswith("embedder.") and leaf in ("bias", "running_mean"):
                v.copy_(0.2 + 0.4 * torch.rand(v.shape, generator=g))
            elif leaf != "num_batches_tracked":
                v.copy_((torch.rand(v.shape, generator=g) - 0.5) * 0.2)
    images = torch.rand(2, 1, 8, 10 * (5 + 2), generator=g)
    gy = torch.randn(2, 5, 32, generator=g)
    # float64 autograd of the yardstick, BatchNorm on batch statistics
    init = {k: v.detach().double().clone() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    with torch.no_grad():
        emb = V.extractor64({k: v.clone() for k, v in init.items()}, images.double(), slice_w=10, training=True,
                            return_embed=True, **cfg)
    assert float((emb != 0).double().mean()) >= V.ALIVE_MIN
    sd = {k: v.clone() for k, v in init.items()}
    names = [k for k, _ in m.named_parameters()]
    for k in names:
        sd[k].requires_grad_(True)
    ref = V.extractor64(sd, images.double(), slice_w=10, training=True, **cfg)
    (ref * gy.double()).sum().backward()
    # the HIP training path
    m = m.to(device).train().set_compute_dtype(torch.float32)
    out = m.train_run(images.to(device), torch.float32)
    (out * gy.to(device)).sum().backward()
    errs = {"out": rel_l2(out.detach().cpu(), ref.detach())}
    for k, p in m.named_parameters():
        sib = k[:-len("bias")] + "weight"
        if norm and k.endswith(".bias") and sd[k].dim() == 1 and sd[sib].dim() == 4:
            # a conv bias under a batch-statistics BatchNorm: the mean subtraction removes it, its gradient is
            # exactly zero (float64 autograd leaves ~1e-17 of rounding).  A relative error of zero means nothing,
            # so the bar is 1e-5 of the scale of the same conv's weight gradient.
            assert float(sd[k].grad.norm()) < 1e-12 * float(sd[sib].grad.norm())
            errs[k] = float(p.grad.norm()) / float(sd[sib].grad.norm())
            continue
        # every other gradient on its own norm -- the first BatchNorm's affine too, although the second BatchNorm
        # all but undoes a change of scale or shift of its input and leaves d gamma_1 a remainder of cancelling
        # terms (sum |dy xhat| = 1700 |d gamma_1|): the C = 1 BatchNorm backward and the kh x kw conv sum in double
        errs[k] = rel_l2(p.grad.cpu(), sd[k].grad)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert len(errs) == 1 + len(names) and all(v < 1e-5 for v in errs.values()), errs
    stats_keys = [k for k in sd if "running" in k]
    assert len(stats_keys) == (4 if norm else 0)
    for k in stats_keys:
        got, want = m.state_dict()[k].double().cpu(), sd[k]
        assert float(((got - want).abs() / want.abs()).max()) < 1e-6, (k, got, want)
        assert not torch.equal(want, init[k])  # the step moved them
