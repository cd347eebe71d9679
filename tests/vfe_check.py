"""The float64 yardstick of the glyph encoder front for any configuration in scope, and random cases for it.

``extractor64`` re-derives the reference's VisualFeatureExtractor.forward in float64: slice the strip into the
overlapping context windows, per layer F.conv2d (zero padding at the WINDOW's edges) -> scale / shift (eval
BatchNorm folded, or batch statistics in training mode, or none) -> ReLU, flatten h * win_w + w, bridge Linear
(+ ReLU).  tests/test_vfe_config.py pins it to goldens recorded from the reference class itself.

``stencil_case`` draws the operands of one vo_vfe_stencil_ex call: pixels in [0, 1], taps U(-0.5, 0.5), bias
and shift positive, scale near 1, so that the ReLU stack stays alive; ``stencil64`` gives the float64 result,
the single-layer element bar of tests/conv_check.py (|got - ref| <= 2 (R + 8) 2^-24 A, R = kh kw,
A = (conv(|x|, |w|) + |b|) |scale| + |shift|) and the fraction of nonzero outputs, which every test asserts to
be at least ALIVE_MIN: against a dead stack every comparison would pass.
"""

import numpy as np
import torch
import torch.nn.functional as F

ALIVE_MIN = 0.25
GOLDEN_CASES = ("s3_k33_l3", "s1_k53_l2", "s2_k35_l1", "s3_k11_l4")


def n_windows(W, slice_w, stride):
    """The reference's slice count (scripts/model/visual_feature_extractor.py:67)."""
    return int((W - (stride // 2) * slice_w * 2) / slice_w)


def windows(images, slice_w, stride):
    """(B, 1, H, W) -> (B n, 1, H, slice_w stride): window i = columns [i slice_w, i slice_w + slice_w stride)."""
    B, C, H, W = images.shape
    n = n_windows(W, slice_w, stride)
    win = torch.stack([images[..., i * slice_w:i * slice_w + slice_w * stride] for i in range(n)], dim=1)
    return win.reshape(B * n, C, H, slice_w * stride), n


# ------------------------------------------------------------------------------------ the stencil alone

def stencil_case(seed, B, H, slice_w, stride, n, kh, kw, layers, extra_w=0):
    """Operands of one vo_vfe_stencil_ex call (CPU, fp32): images (B, 1, H, W) with W = the width n windows
    need + extra_w trailing columns (fewer than slice_w: ignored), conv (layers, kh kw + 1), bn (layers, 2)."""
    assert 0 <= extra_w < slice_w
    g = torch.Generator().manual_seed(seed)
    W = (n + 2 * (stride // 2)) * slice_w + extra_w  # the strip with pad_2D_gray_image's margins
    assert n_windows(W, slice_w, stride) == n
    images = torch.rand(B, 1, H, W, generator=g)
    c = dict(images=images, slice_w=slice_w, stride=stride, kernel=(kh, kw), n=n, H=H,
             name=f"B{B}_H{H}_sw{slice_w}_s{stride}_n{n}_k{kh}x{kw}_l{layers}" + (f"_x{extra_w}" if extra_w else ""))
    conv, bn = torch.empty(0, kh * kw + 1), torch.empty(0, 2)
    for _ in range(layers):
        # one layer at a time, redrawn (same generator: deterministic) until half of ITS float64 outputs are
        # nonzero: taps of either sign can add up to a negative response everywhere, and a dead layer would hide
        # every layer after it.  The choice looks at the float64 reference only.
        for _ in range(64):
            taps = torch.rand(1, kh * kw, generator=g) - 0.5
            bias = 0.2 + 0.4 * torch.rand(1, 1, generator=g)
            scale = 0.7 + 0.6 * torch.rand(1, 1, generator=g)
            shift = 0.1 + 0.4 * torch.rand(1, 1, generator=g)
            c["conv"] = torch.cat([conv, torch.cat([taps, bias], 1)]).contiguous()
            c["bn"] = torch.cat([bn, torch.cat([scale, shift], 1)]).contiguous()
            if stencil64(c)[2] >= 0.5:
                break
        else:
            raise AssertionError(f"{c['name']}: no live layer in 64 draws")
        conv, bn = c["conv"], c["bn"]
    return c


def stencil64(c):
    """(ref (B n, H win_w), bar or None, alive): float64 result of the case; the element bar for one layer."""
    kh, kw = c["kernel"]
    x, n = windows(c["images"].double(), c["slice_w"], c["stride"])
    assert n == c["n"]
    A = None
    for l in range(c["conv"].shape[0]):
        w = c["conv"][l, :kh * kw].double().view(1, 1, kh, kw)
        b = c["conv"][l, kh * kw:].double()
        sc, sh = c["bn"][l].double()
        if l == 0:
            A = (F.conv2d(x.abs(), w.abs(), b.abs(), padding=((kh - 1) // 2, (kw - 1) // 2))) * sc.abs() + sh.abs()
        x = torch.relu(F.conv2d(x, w, b, padding=((kh - 1) // 2, (kw - 1) // 2)) * sc + sh)
    ref = x.reshape(x.shape[0], -1)
    bar = 2 * (kh * kw + 8) * 2.0 ** -24 * A.reshape(ref.shape) if c["conv"].shape[0] == 1 else None
    return ref, bar, float((ref != 0).double().mean())


# ------------------------------------------------------------------------------------ the whole module

def layer_keys(layers, norm):
    """[(conv index, BatchNorm index or None)] in the embedder Sequential."""
    step = 3 if norm else 2
    return [(l * step, l * step + 1 if norm else None) for l in range(layers)]


def extractor64(sd, images, *, slice_w, stride, kernel, layers, norm, relu, training=False, eps=1e-5, momentum=0.1,
                return_embed=False):
    """sd: {state-dict key: float64 tensor} of a VisualFeatureExtractor (embedder.<i>.*, bridge.0.* or bridge.*).
    training: BatchNorm with batch statistics; the running statistics in ``sd`` are updated in place as
    torch does (momentum, unbiased variance)."""
    kh, kw = kernel
    x, n = windows(images, slice_w, stride)
    for ci, bi in layer_keys(layers, norm):
        x = F.conv2d(x, sd[f"embedder.{ci}.weight"], sd[f"embedder.{ci}.bias"], padding=((kh - 1) // 2, (kw - 1) // 2))
        if bi is not None:
            x = F.batch_norm(x, sd[f"embedder.{bi}.running_mean"], sd[f"embedder.{bi}.running_var"],
                             sd[f"embedder.{bi}.weight"], sd[f"embedder.{bi}.bias"], training, momentum, eps)
        x = torch.relu(x)
    if return_embed:
        return x
    p = "bridge.0." if relu else "bridge."
    y = F.linear(x.reshape(x.shape[0], -1), sd[p + "weight"], sd[p + "bias"])
    if relu:
        y = torch.relu(y)
    return y.view(images.shape[0], n, -1)


def golden_config(g):
    """The configuration recorded in a vfe_cfg_<name>.npz and its state dict as fp32 arrays."""
    cfg = dict(stride=int(g["stride"]), kernel=tuple(int(v) for v in g["kernel"]), layers=int(g["layers"]),
               norm=bool(g["embed_normalize"]), relu=bool(g["bridge_relu"]))
    sd = {k[3:]: np.array(g[k]) for k in g.files if k.startswith("sd.")}
    return cfg, sd


def build_module(cfg, slice_w, slice_h, embed):
    from visual_onoma_to_wave_amd.model.visual_feature_extractor import VisualFeatureExtractor
    return VisualFeatureExtractor("gray-scale", slice_w, slice_h, embed, cfg["stride"], embed_normalize=cfg["norm"],
                                  bridge_relu=cfg["relu"], kernel_size=cfg["kernel"], num_convolutions=cfg["layers"])


# ------------------------------------------------------------------------------------ the GPU cases
# (B, H, slice_w, stride, n windows, kh, kw, trailing columns) -- the smallest shapes at which each mechanism of
# vo_vfe_stencil_ex can fail; tests/test_vfe_config.py checks on the CPU that each keeps its ReLU stack alive at
# every depth.  3 x 3 at stride 1 and slice_w <= 128 is dispatched to the ICASSP kernel, every other line to
# the window kernel.

SHAPES = [
    # window isolation: overlapping windows, odd and even stride (the even-stride margin)
    (2, 4, 5, 3, 4, 3, 3, 0), (2, 4, 5, 2, 3, 3, 3, 0),
    # window smaller than the kernel: H = 3, win_w = 4 under 7 x 9 taps
    (1, 3, 4, 1, 2, 7, 9, 0), (1, 3, 2, 2, 2, 7, 9, 0),
    # non-square kernels on H = 5, slice_w = 6, stride 1 and 3
    *[(2, 5, 6, s, 3, kh, kw, 0) for s in (1, 3) for kh, kw in ((1, 1), (1, 7), (7, 1), (3, 5), (5, 3))],
    # the widest taps, and an even stride under them
    (1, 6, 7, 2, 2, 9, 9, 0), (2, 5, 6, 1, 2, 5, 5, 0),
    # H * win_w below / not a multiple of the workgroup size
    # (the 3 x 3 ragged shape at stride 1 runs the ICASSP kernel, at stride 2 the window kernel)
    (2, 1, 1, 1, 3, 5, 3, 0), (2, 5, 13, 1, 2, 3, 3, 0), (2, 5, 13, 2, 2, 3, 3, 0), (2, 5, 13, 1, 2, 3, 7, 0),
    (1, 24, 102, 3, 2, 3, 3, 0),
    # W not a multiple of slice_w: the trailing columns are ignored
    (2, 5, 6, 3, 3, 3, 3, 4), (2, 5, 6, 1, 3, 5, 3, 5),
    # a single window, W = win_w exactly
    (1, 5, 6, 3, 1, 3, 5, 0),
]
DEPTHS = (1, 2, 3, 4)  # the ping-pong ends in either buffer


def shape_case(shape, layers):
    B, H, sw, s, n, kh, kw, extra = shape
    seed = (B * 7919 + H * 104729 + sw * 1299709 + s * 15485863 + n * 31 + kh * 7 + kw * 3 + extra + layers * 977) % 2 ** 31
    return stencil_case(seed, B, H, sw, s, n, kh, kw, layers, extra)


def shape_id(shape):
    B, H, sw, s, n, kh, kw, extra = shape
    return f"B{B}-H{H}-sw{sw}-s{s}-n{n}-k{kh}x{kw}" + (f"-x{extra}" if extra else "")
