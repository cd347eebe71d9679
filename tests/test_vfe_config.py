"""The glyph encoder's config surface on the host: the LDS query of vo_vfe_stencil_ex, the state-dict layout
under visual_text.stride / conv_kernel_size / layer_num, what VisualFeatureExtractor._supported accepts and
refuses, and the float64 yardstick of tests/vfe_check.py pinned to goldens recorded from the reference's own
VisualFeatureExtractor (tests/golden/make_goldens_vfe.py).  No GPU: the query makes no HIP call."""

import copy
import itertools

import pytest
import torch

import vfe_check as V
from helpers import configs, golden, rel_l2, spec
from weights import spec_of

KIB = 1024


def _lds(H, win_w, kh, kw):
    from visual_onoma_to_wave_amd import ops
    return ops.vfe_stencil_lds_bytes(H, win_w, kh, kw)


def test_lds_bytes_of_the_documented_windows():
    assert 0 < _lds(24, 102, 3, 3) <= 64 * KIB
    assert _lds(24, 306, 3, 3) <= 160 * KIB  # stride 3
    assert _lds(24, 510, 3, 3) <= 160 * KIB  # stride 5
    # two copies of the window and its zero border, fp32: never less than that
    for H, w, kh, kw in ((24, 102, 3, 3), (24, 306, 3, 3), (8, 30, 5, 3), (1, 1, 1, 1), (32, 128, 9, 9)):
        assert _lds(H, w, kh, kw) >= 2 * (H + kh - 1) * (w + kw - 1) * 4, (H, w, kh, kw)


def test_lds_bytes_monotone_in_every_argument():
    Hs, ws, ks = (1, 2, 7, 8, 23, 24, 25, 32), (1, 3, 4, 5, 101, 102, 103, 305, 306, 307, 510), (1, 3, 5, 7, 9)
    for H, w, kh, kw in itertools.product(Hs, ws, ks, ks):
        here = _lds(H, w, kh, kw)
        assert here > 0
        assert _lds(H + 1, w, kh, kw) >= here and _lds(H, w + 1, kh, kw) >= here, (H, w, kh, kw)
        if kh < 9:
            assert _lds(H, w, kh + 2, kw) >= here, (H, w, kh, kw)
        if kw < 9:
            assert _lds(H, w, kh, kw + 2) >= here, (H, w, kh, kw)
    # and strictly over a whole 16-byte chunk of columns or a row
    assert _lds(24, 310, 3, 3) > _lds(24, 306, 3, 3) and _lds(25, 306, 3, 3) > _lds(24, 306, 3, 3)
    assert _lds(24, 306, 5, 3) > _lds(24, 306, 3, 3) and _lds(24, 306, 3, 3) > _lds(24, 306, 3, 1)


def test_random_cases_stay_alive_and_fit():
    """Every case the GPU tests draw: at least a quarter of the last layer's float64 outputs nonzero (a dead
    ReLU stack would make every comparison pass), and the window inside the LDS bound."""
    assert (1, 24, 102, 3, 2, 3, 3, 0) in V.SHAPES  # the ICASSP glyph at stride 3
    for shape in V.SHAPES:
        B, H, sw, s, n, kh, kw, extra = shape
        assert _lds(H, sw * s, kh, kw) <= 160 * KIB
        for layers in V.DEPTHS:
            c = V.shape_case(shape, layers)
            ref, bar, alive = V.stencil64(c)
            assert ref.shape == (B * n, H * sw * s) and (bar is None) == (layers > 1)
            assert alive >= V.ALIVE_MIN, (c["name"], alive)


def test_state_dict_layout_stride3_matches_spec():
    from visual_onoma_to_wave_amd.model import vTTS
    pc, mc, tc = configs()
    pc = copy.deepcopy(pc)
    pc["visual_text"]["stride"] = 3
    m = vTTS(pc, mc, tc)
    _, want = spec("vtts_s3")
    got = [(k, tuple(s), t) for k, s, t in spec_of(m.state_dict())]
    assert got == want
    _, base = spec("vtts")
    diff = [(a, b) for a, b in zip(base, want) if a != b]
    assert len(base) == len(want) and len(diff) == 1
    assert diff[0][1][0] == "encoder.VisualFeatureExtractor.bridge.0.weight" and diff[0][1][1] == (256, 7344)


def test_state_dict_layout_kernel_5x3_two_layers():
    m = V.build_module(dict(stride=1, kernel=(5, 3), layers=2, norm=True, relu=True), 10, 8, 32)
    sd = m.state_dict()
    assert tuple(sd["embedder.0.weight"].shape) == (1, 1, 5, 3) and tuple(sd["embedder.3.weight"].shape) == (1, 1, 5, 3)
    assert len(m.embedder) == 2 * 3
    assert [type(x).__name__ for x in m.embedder] == ["Conv2d", "BatchNorm2d", "ReLU"] * 2
    assert tuple(m.embedder[0].padding) == (2, 1)
    assert tuple(sd["bridge.0.weight"].shape) == (32, 8 * 10)
    m._supported()  # and the HIP path takes that layout


# (the ICASSP configuration -- stride 1, 3 x 3, 3 layers, BatchNorm, bridge ReLU -- is what every earlier test runs)
IN_SCOPE = [dict(stride=s, kernel=k, layers=l, norm=nm, relu=r)
            for s, k, l, nm, r in [(3, (3, 3), 3, True, True), (2, (3, 5), 1, True, True),
                                   (1, (5, 3), 2, True, True), (3, (1, 1), 4, False, False), (5, (3, 3), 3, True, True),
                                   (1, (9, 9), 1, True, False), (1, (1, 9), 2, False, True), (4, (7, 1), 5, True, True),
                                   (1, (3, 3), 1, False, True), (1, (3, 3), 2, True, False)]]


@pytest.mark.parametrize("cfg", IN_SCOPE, ids=lambda c: f"s{c['stride']}k{c['kernel'][0]}{c['kernel'][1]}l{c['layers']}"
                                                        f"{'n' if c['norm'] else ''}{'r' if c['relu'] else ''}")
def test_supported_accepts_the_scope(cfg):
    V.build_module(cfg, 102, 24, 256)._supported()
    V.build_module(cfg, 10, 8, 32)._supported()


def test_supported_refuses_outside_the_scope():
    from visual_onoma_to_wave_amd.model.visual_feature_extractor import VisualFeatureExtractor as VFE
    with pytest.raises(NotImplementedError, match="gray-scale"):
        VFE("RGB-scale", 102, 24, 256, 1, kernel_size=(3, 3), num_convolutions=3)._supported()
    for k in ((11, 3), (3, 11)):
        with pytest.raises(NotImplementedError, match="from 1 to 9"):
            VFE("gray-scale", 102, 24, 256, 1, kernel_size=k, num_convolutions=1)._supported()
    # a window over the LDS bound, found through the query: the first stride whose window the query prices above it
    stride = next(s for s in range(1, 64) if _lds(24, 102 * s, 3, 3) > 160 * KIB)
    assert _lds(24, 102 * (stride - 1), 3, 3) <= 160 * KIB and stride > 5
    VFE("gray-scale", 102, 24, 256, stride - 1, kernel_size=(3, 3), num_convolutions=3)._supported()
    with pytest.raises(NotImplementedError, match="LDS"):
        VFE("gray-scale", 102, 24, 256, stride, kernel_size=(3, 3), num_convolutions=3)._supported()
    # the bridge runs as a conv over H * win_w input channels: a multiple of 8
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        VFE("gray-scale", 10, 7, 32, 3, kernel_size=(3, 3), num_convolutions=1)._supported()


def test_vfe_conv_refuses_with_the_limits():
    from visual_onoma_to_wave_amd import autograd as AG
    x = torch.zeros(1, 1, 4, 4)
    for conv in (torch.nn.Conv2d(1, 1, (11, 3), padding=(5, 1)), torch.nn.Conv2d(1, 1, (5, 3), padding=(1, 1)),
                 torch.nn.Conv2d(1, 1, (3, 5), padding=(1, 2), bias=False), torch.nn.Conv2d(2, 2, 3, padding=1),
                 torch.nn.Conv2d(1, 1, (3, 5), padding=(1, 2), stride=2)):
        with pytest.raises(NotImplementedError, match="odd kh, kw <= 9"):
            AG.vfe_conv(x, conv)


@pytest.mark.parametrize("name", V.GOLDEN_CASES)
def test_yardstick_is_the_reference_computation(name):
    """extractor64 on the golden's fp32 parameters and images against the reference's fp32 output: rel-L2 < 1e-6,
    the distance of an fp32 result from float64."""
    g = golden("vfe_cfg_" + name)
    cfg, sd = V.golden_config(g)
    assert name == f"s{cfg['stride']}_k{cfg['kernel'][0]}{cfg['kernel'][1]}_l{cfg['layers']}"
    images = torch.from_numpy(g["images"])
    assert tuple(images.shape) == (2, 1, 8, 10 * (5 + cfg["stride"] - 1)) and 0.0 < float(images.std())
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items() if v.dtype.kind == "f"}
    out = V.extractor64(sd64, images.double(), slice_w=10, **cfg)
    e = rel_l2(out, g["out"])
    print(f"{name}: yardstick vs reference rel-L2 {e:.3e}")
    assert out.shape == g["out"].shape and e < 1e-6
    emb = V.extractor64(sd64, images.double(), slice_w=10, return_embed=True, **cfg)
    assert float((emb != 0).double().mean()) >= V.ALIVE_MIN
    # the module takes the golden's state dict as it is: keys, order and shapes
    m = V.build_module(cfg, 10, 8, 32)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == \
        [(k[3:], tuple(g[k].shape)) for k in g.files if k.startswith("sd.")]
