"""Glyph stretching on the GPU: ``vo_glyph_stretch`` through ``ops.glyph_stretch`` and
``dataset.GlyphAtlas`` against the numpy model of tests/glyph_stretch_check.py (pinned on the host against Pillow,
tests/test_glyph_stretch_cpu.py), against ``GlyphBatch`` on strips Pillow resized, against the committed golden, and
inside ``pipeline.GraphedSynthesis``.  The output is uint8 / 255: every comparison is ``torch.equal``."""

import numpy as np
import pytest
import torch

import glyph_stretch_check as C
import graphed_case as G
from helpers import configs, golden, hifigan_arrays, hifigan_h, vtts_arrays
from weights import load_into

pytestmark = pytest.mark.gpu

BATCH, MAX_SRC, CAP, HOP, SCALE = G.BATCH, G.MAX_SRC, G.CAP, G.HOP, G.PCM_SCALE


def _atlas(glyphs, cell, stride, device):
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    return GlyphAtlas(glyphs, cell, stride).to(device)


def _pil_batch(glyphs, ids, lens, widths, cell, stride):
    """The strips a notebook user builds: every character resized by Pillow and pasted side by side."""
    from visual_onoma_to_wave_amd.dataset import GlyphBatch
    H = glyphs.shape[1]
    strips, cw = [], []
    for b in range(len(ids)):
        n = int(lens[b])
        cols = [C.pil_resize(glyphs[ids[b][t]], widths[b][t]) for t in range(n)]
        strips.append(np.concatenate(cols, axis=1) if cols else np.zeros((H, 0), np.uint8))
        cw.append(np.asarray(widths[b][:n]))
    return GlyphBatch(strips, cw, cell, stride)


def _every_width(device, H, S, cell, B, T, stride, seed):
    """B * T = cell cells carrying the widths 1 .. cell in one launch, full rows."""
    assert B * T == cell
    rng = np.random.default_rng(seed)
    glyphs = C.random_glyphs(seed, 9, H, S)
    glyphs[5:] = C.random_glyphs(seed + 1, 4, H, S, binary=True)
    ids = rng.integers(0, 9, size=(B, T)).astype(np.int64)
    widths = rng.permutation(np.arange(1, cell + 1)).reshape(B, T).astype(np.int32)
    lens = np.full(B, T, np.int64)
    atlas = _atlas(glyphs, cell, stride, device)
    got = atlas.layout(ids, lens, widths)
    assert got.dtype == torch.float32 and got.shape == (B, 1, H, (T + 2 * (stride // 2)) * cell)
    ref = C.layout(glyphs, ids, lens, widths, cell, atlas.margin)
    assert torch.equal(got.cpu(), torch.from_numpy(ref)), "differs from the numpy model"
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    pil = _pil_batch(glyphs, ids, lens, widths, cell, stride).to(device, n_chars=T)
    assert torch.equal(got, pil), "differs from GlyphBatch on strips Pillow resized"


def test_every_width_in_one_launch(device):
    _every_width(device, 24, 24, 102, 6, 17, 1, seed=7)


def test_second_geometry(device):
    """Nothing of 24 or 102 is built in: 16 x 16 glyphs in 40-pixel cells, with a stride-3 margin."""
    _every_width(device, 16, 16, 40, 4, 10, 3, seed=8)


def test_height_that_is_no_multiple_of_the_row_group(device):
    """13 rows of 11 pixels in 30-pixel cells: the last group of rows of a cell is partial (8 + 5), nothing is
    square, and the record pitch (13) is already odd."""
    _every_width(device, 13, 11, 30, 3, 10, 2, seed=9)


EDGE_WIDTHS =(0, -3, 1, 2, 12, 23, 24, 25, 101, 102, 103, 1000)


def test_edge_cases_every_element_written(device):
    """Widths at and past both ends, ids at and past both ends of the atlas, lengths 0, 2 and T, a stride-3 margin and
    a W_out wider than needed, into an ``out`` pre-filled with NaN."""
    from visual_onoma_to_wave_amd import ops
    B, T, H, S, cell, stride = 3, 5, 24, 24, 102, 3
    n_glyphs = 4
    glyphs = C.random_glyphs(21, n_glyphs, H, S)
    atlas = _atlas(glyphs, cell, stride, device)
    margin = atlas.margin
    assert margin == 102
    W_out = T * cell + 2 * margin + 37
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)  # noqa: E731
    pool = np.asarray(list(EDGE_WIDTHS) + [24, 1, 102], np.int32).reshape(B, T)
    drawn, parity = set(), set()
    for rot in range(B):  # each row of widths is the full-length row once
        full, two, empty = rot, (rot + 1) % B, (rot + 2) % B
        lens = np.zeros(B, np.int64)
        lens[full], lens[two], lens[empty] = T, 2, 0
        ids = np.random.default_rng(rot).integers(1, n_glyphs, size=(B, T)).astype(np.int64)
        ids[full, rot] = 0                       # the first glyph: drawn
        ids[two, 0], ids[two, 1] = -1, n_glyphs  # live cells whose id is past either end: white
        ids[empty, 2] = 1 << 40                  # past the length anyway
        drawn.update(int(w) for w in pool[full])
        parity.update((cell - min(int(w), cell)) % 2 for w in pool[full] if w > 0)
        out = torch.full((B, 1, H, W_out), float("nan"), device=device)
        got = ops.glyph_stretch(atlas.glyphs_d, atlas.table_d, dev(ids, np.int64), dev(lens, np.int64),
                                dev(pool, np.int32), cell, margin, W_out=W_out, out=out)
        assert got is out and not torch.isnan(out).any(), f"rotation {rot}: elements left unwritten"
        ref = C.layout(glyphs, ids, lens, pool, cell, margin, W_out)
        assert torch.equal(out.cpu(), torch.from_numpy(ref)), f"rotation {rot}"
        assert bool((out[two, ..., :margin + 2 * cell] == 1.0).all()), "ids -1 and n_glyphs are white cells"
        # widths = NULL: every glyph as it is, on the same ids and lengths
        out.fill_(float("nan"))
        ops.glyph_stretch(atlas.glyphs_d, atlas.table_d, dev(ids, np.int64), dev(lens, np.int64), None, cell, margin,
                          W_out=W_out, out=out)
        ref = C.layout(glyphs, ids, lens, None, cell, margin, W_out)
        assert torch.equal(out.cpu(), torch.from_numpy(ref)), f"rotation {rot}, widths = None"
    assert drawn >= set(EDGE_WIDTHS) and parity == {0, 1}


def test_device_tensors_and_host_arrays_agree(device):
    """``layout`` on validated host arrays and on device tensors (unread) is one launch on the same values; n_chars
    widens with white."""
    glyphs = C.random_glyphs(31, 5, 24, 24)
    atlas = _atlas(glyphs, 102, 1, device)
    ids = np.array([[1, 2, 3, 4], [4, 3, 0, 0]], np.int64)
    lens = np.array([4, 2], np.int64)
    widths = np.array([[10, 24, 77, 102], [0, 50, 0, 0]], np.int32)
    a = atlas.layout(ids, lens, widths, n_chars=6)
    b = atlas.layout(torch.from_numpy(ids).to(device), torch.from_numpy(lens).to(device),
                     torch.from_numpy(widths).to(device), n_chars=6)
    ref = C.layout(glyphs, ids, lens, widths, 102, 0, 6 * 102)
    assert a.shape == (2, 1, 24, 612) and torch.equal(a, b) and torch.equal(a.cpu(), torch.from_numpy(ref))
    assert bool((a[..., 4 * 102:] == 1.0).all())


def test_committed_golden(device):
    g = golden("glyph_stretch")
    cell, stride = int(g["cell"]), int(g["stride"])
    atlas = _atlas(g["glyphs"], cell, stride, device)
    got = atlas.layout(g["ids"], g["lens"], g["widths"])
    assert torch.equal(got.cpu(), torch.from_numpy(g["expected"]))


# ------------------------------------------------------------------------------ GraphedSynthesis

@pytest.fixture(scope="module")
def vtts(device):
    from test_gpu_graphed_synthesis import _bias_shift
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    m = m.to(device).eval()
    m.set_precision("mixed")
    with _bias_shift(m, G.DUR_BIAS_SHIFT):
        yield m


@pytest.fixture(scope="module")
def gen(device):
    from visual_onoma_to_wave_amd import hifigan
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    g = g.to(device)
    g.set_compute_dtype(torch.bfloat16)
    return g


@pytest.fixture(scope="module")
def atlas73(device):
    """73 symbols (ids 0 .. 72 of the packaged vocabulary): seeded black-on-white glyphs, PAD white."""
    glyphs = C.random_glyphs(73, 73, 24, 24, binary=True)
    glyphs[0] = 255
    return _atlas(glyphs, 102, 1, device)


def _gs(vtts, gen, **kw):
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    return GraphedSynthesis(vtts, gen, BATCH, MAX_SRC, CAP, pcm_scale=SCALE, **kw)


def _req(i):
    r = G.request_set(i)
    return {k: r[k] for k in ("audiotypes", "src_lens", "texts", "e_control", "d_control")}


def _widths(seed):
    return np.random.default_rng(seed).integers(6, 103, size=(BATCH, MAX_SRC)).astype(np.int32)


def _snapshot(res):
    torch.cuda.synchronize()
    return res.wav.clone(), res.samples.clone(), res.mel_len.clone()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("wav", "samples", "mel_len")):
        assert x.dtype == y.dtype and torch.equal(x, y), f"{what}: {name} differs"


def test_graphed_atlas_equals_graphed_images(vtts, gen, atlas73, device):
    gs_a, gs_i = _gs(vtts, gen, atlas=atlas73), _gs(vtts, gen)
    assert gs_a.inputs.widths.dtype == torch.int32 and gs_a.inputs.widths.shape == (BATCH, MAX_SRC)
    assert gs_i.inputs.widths is None and gs_i.atlas is None
    for i in range(2):
        q, w = _req(i), _widths(40 + i)
        a = _snapshot(gs_a(**q, widths=w))
        assert a[0].dtype == torch.int16 and a[0].shape == (BATCH, CAP * HOP)
        images = atlas73.layout(q["texts"], q["src_lens"], w, n_chars=MAX_SRC)
        assert torch.equal(gs_a.inputs.images, images)
        b = _snapshot(gs_i(**q, images=images))
        _same(a, b, f"set {i}")
        assert int(a[1].min()) > 0, "the utterances are not empty"
    # n < batch: the rows past n are copies of request 0, widths included
    q, w = _req(2), _widths(42)
    part = {k: (v[:2] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == BATCH else v) for k, v in q.items()}
    res = gs_a(**part, widths=w[:2])
    assert res.wav.shape[0] == 2
    a = _snapshot(res)
    assert torch.equal(gs_a.inputs.widths[2], gs_a.inputs.widths[0])
    assert torch.equal(gs_a.inputs.images[2], gs_a.inputs.images[0])
    images = atlas73.layout(q["texts"][:2], q["src_lens"][:2], w[:2], n_chars=MAX_SRC)
    _same(a, _snapshot(gs_i(**part, images=images)), "n = 2")
    assert gs_a.captures == 1 and gs_i.captures == 1


def test_replay_follows_widths_and_glyphs_changed_in_place(vtts, gen, device):
    glyphs = C.random_glyphs(74, 73, 24, 24, binary=True)
    atlas = _atlas(glyphs, 102, 1, device)  # its own: a glyph is edited below
    gs = _gs(vtts, gen, atlas=atlas)
    q = _req(0)
    first = _snapshot(gs(**q, widths=_widths(50)))
    images0 = gs.inputs.images.clone()
    new = _widths(51)
    gs.inputs.widths.copy_(torch.from_numpy(new).to(device))
    gs.graph.replay()
    torch.cuda.synchronize()
    out, wav, samples, _ = gs._out
    replayed = (wav.clone(), samples.clone(), out[9].clone())
    assert not torch.equal(gs.inputs.images, images0), "the replay drew the new widths"
    fresh = _snapshot(gs(**q, widths=new))
    _same(replayed, fresh, "replay after widths.copy_")
    assert not torch.equal(first[0], fresh[0]), "the widths are heard"
    # widths = None: every glyph at its own width S
    none = _snapshot(gs(**q))
    assert bool((gs.inputs.widths == 24).all())
    _same(none, _snapshot(gs(**q, widths=np.full((BATCH, MAX_SRC), 24, np.int32))), "widths=None")
    # a glyph edited in place in the atlas
    sym = int(q["texts"][0, 0])
    images1 = gs.inputs.images.clone()
    atlas.glyphs_d[sym] = 255 - atlas.glyphs_d[sym]
    gs.graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(gs.inputs.images, images1)
    glyphs2 = glyphs.copy()
    glyphs2[sym] = 255 - glyphs2[sym]
    ref = C.layout(glyphs2, q["texts"], q["src_lens"], None, 102, 0)
    assert torch.equal(gs.inputs.images.cpu(), torch.from_numpy(ref))
    assert gs.captures == 1


def test_graphed_atlas_refusals(vtts, gen, atlas73, device):
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    g = atlas73.glyphs
    with pytest.raises(ValueError, match="atlas must be on"):
        _gs(vtts, gen, atlas=GlyphAtlas(g, 102, 1))
    for bad in (GlyphAtlas(g, 100, 1), GlyphAtlas(g, 102, 3), GlyphAtlas(g[:, :16], 102, 1)):
        with pytest.raises(ValueError, match="does not match"):
            _gs(vtts, gen, atlas=bad.to(device))
    with pytest.raises(ValueError, match="use_image=True"):
        _gs(vtts, gen, atlas=atlas73, use_image=False)
    gs = _gs(vtts, gen, atlas=atlas73)
    q = _req(0)
    before = gs.inputs.texts.clone()
    images = torch.ones((BATCH, 1, 24, MAX_SRC * 102), device=device)
    with pytest.raises(ValueError, match="(?s)atlas.*texts.*images"):
        gs(q["audiotypes"], q["src_lens"], images, texts=q["texts"])
    with pytest.raises(ValueError, match="needs texts"):
        gs(q["audiotypes"], q["src_lens"])
    with pytest.raises(ValueError, match="widths must be in"):
        gs(**q, widths=np.full((BATCH, MAX_SRC), 103, np.int32))
    with pytest.raises(ValueError, match="texts must be in"):
        gs(**dict(q, texts=np.full((BATCH, MAX_SRC), 73, np.int64)))
    with pytest.raises(ValueError, match="widths must have shape"):
        gs(**q, widths=np.full((BATCH, MAX_SRC + 1), 24, np.int32))
    assert gs.captures == 0 and torch.equal(gs.inputs.texts, before), "a refused call changes nothing"
    with pytest.raises(ValueError, match="widths need an atlas"):
        _gs(vtts, gen)(q["audiotypes"], q["src_lens"], images, widths=_widths(1))


def test_without_atlas_images_equal_eager_as_before(vtts, gen, device):
    from test_gpu_graphed_synthesis import _assert_equal, _eager, _request
    gs = _gs(vtts, gen)
    q = _request(0)
    res = gs(**q)
    out, wav = _eager(vtts, gen, q, SCALE)
    _assert_equal(res, out, wav, what="no atlas")
    assert gs.captures == 1
