"""Glyph stretching on the host: the coefficient table of ``vo_glyph_stretch_table`` against
the numpy model of tests/glyph_stretch_check.py, that model against Pillow's own resize and against the committed
golden (Pillow's resize + the oracle's layout), the reference's two integer width rules, the PIL atlas renderer and
the host-side validation.  No GPU call is made."""

import ctypes

import numpy as np
import pytest

import glyph_stretch_check as C
from helpers import configs, golden

GEOMETRIES = C.GEOMETRIES


# ------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("S,cell", GEOMETRIES)
def test_table_equals_model_record_for_record(S, cell):
    from visual_onoma_to_wave_amd import ops
    got, ref = ops.glyph_stretch_table(S, cell), C.table(S, cell)
    assert got.dtype == np.int32 and got.shape == ref.shape == (cell * (cell + 1) // 2, 2 + S)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} records differ, the first: {bad[0]}: {got[bad[0]]} vs {ref[bad[0]]}"
    if (S, cell) == (24, 102):
        assert got.nbytes == 546312


@pytest.mark.parametrize("S,cell", GEOMETRIES)
def test_table_facts(S, cell):
    """n <= S with taps inside the glyph, zeros past n, w = S the identity, and int32 holds every sum."""
    tab = C.table(S, cell)
    xmin, n = tab[:, 0], tab[:, 1]
    assert (xmin >= 0).all() and (n >= 1).all() and (n <= S).all() and (xmin + n <= S).all()
    for r in tab:
        assert not r[2 + r[1]:].any()
    ident = tab[S * (S - 1) // 2:S * (S - 1) // 2 + S]
    for c, r in enumerate(ident):
        K = np.zeros(S, np.int64)
        K[r[0]:r[0] + r[1]] = r[2:2 + r[1]]
        assert K[c] == 1 << C.BITS and not np.delete(K, c).any(), (c, r)
    g = C.random_glyphs(5, 1, S, S)[0]
    assert np.array_equal(C.resize(g, S, tab), g)
    # the extreme of 2^21 + sum src K over src in [0, 255], and the looser sum |K| form
    exact = C.acc_bound(tab)
    loose = (1 << (C.BITS - 1)) + 255 * int(np.abs(tab[:, 2:].astype(np.int64)).sum(axis=1).max())
    print(f"S = {S}, cell = {cell}: |acc| <= {exact} (sum |K| form: {loose})")
    assert exact <= loose < 2 ** 31
    if S == 24:
        assert loose <= 1_358_585_972


def test_table_entries_refuse_bad_sizes_and_short_buffers():
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    for S, cell in ((0, 10), (65, 10), (24, 0), (24, 257), (-1, -1)):
        assert L.vo_glyph_stretch_table_size(S, cell) == -1
        buf = np.zeros(16, np.int32)
        assert L.vo_glyph_stretch_table(S, cell, ctypes.c_void_p(buf.ctypes.data), buf.nbytes) != 0
        assert b"glyph_stretch_table" in L.vo_last_error()
        with pytest.raises(ValueError, match="src_w must be in"):
            ops.glyph_stretch_table(S, cell)
    assert L.vo_glyph_stretch_table_size(64, 256) == 256 * 257 // 2 * 66 * 4
    need = L.vo_glyph_stretch_table_size(16, 40)
    assert need == 59040
    buf = np.full(need // 4 + 3, 7, np.int32)
    assert L.vo_glyph_stretch_table(16, 40, ctypes.c_void_p(buf.ctypes.data), need - 1) != 0
    assert (buf == 7).all(), "a refused call writes nothing"
    assert L.vo_glyph_stretch_table(16, 40, None, need) != 0
    assert L.vo_glyph_stretch_table(16, 40, ctypes.c_void_p(buf.ctypes.data), need) == 0
    assert (buf[need // 4:] == 7).all(), "nothing past the table's bytes"
    assert np.array_equal(buf[:need // 4].reshape(-1, 18), C.table(16, 40))


# ------------------------------------------------------------------------------ the model against Pillow

@pytest.mark.parametrize("S,cell", GEOMETRIES)
def test_model_equals_pillow_for_every_width(S, cell):
    pytest.importorskip("PIL")
    tab = C.table(S, cell)
    for binary in (False, True):
        g = C.random_glyphs(11 + S, 1, S, S, binary)[0]
        for w in range(1, cell + 1):
            got, ref = C.resize(g, w, tab), C.pil_resize(g, w)
            assert np.array_equal(got, ref), (f"S = {S}, w = {w}, binary = {binary}: {int((got != ref).sum())} pixels "
                                              f"differ")


def test_model_reproduces_the_golden():
    g = golden("glyph_stretch")
    cell, stride = int(g["cell"]), int(g["stride"])
    assert sorted(g["widths"][g["widths"] > 0].tolist()) == list(range(1, cell + 1)), "every width once"
    got = C.layout(g["glyphs"], g["ids"], g["lens"], g["widths"], cell, (stride // 2) * cell)
    assert got.dtype == np.float32 and got.shape == g["expected"].shape
    assert np.array_equal(got, g["expected"])


# ------------------------------------------------------------------------------ the reference's width rules

def test_widths_from_rates_is_the_notebooks_expression():
    from visual_onoma_to_wave_amd.dataset import widths_from_rates
    rng = np.random.default_rng(3)
    rates = np.concatenate([np.arange(1, 43) * 0.1, rng.uniform(0.05, 4.25, 200), [1.0, 0.0, 4.25]])
    for fs in (24, 16, 32):
        got = widths_from_rates(rates, fs)
        assert got.dtype == np.int32 and got.shape == rates.shape
        assert got.tolist() == [int(fs * rates[i]) for i in range(len(rates))]
    # the notebook's own steps: 1.0 + 0.1 + 0.1 + ... accumulated in float64
    acc, r = [], np.float64(1.0)
    for _ in range(30):
        r = r + 0.1
        acc.append(r)
    assert widths_from_rates(acc, 24).tolist() == [int(24 * v) for v in acc]
    assert widths_from_rates(np.array([[1.0, 0.5], [2.0, 1.25]]), 24).tolist() == [[24, 12], [48, 30]]


def test_allocate_widths_is_the_generators_expression():
    from visual_onoma_to_wave_amd.dataset import allocate_widths
    for n in (1, 2, 5, 7, 12, 21):
        for cw in (n, 24 * n, 24 * n + 1, 24 * n + n - 1, 517, 13):
            got = allocate_widths(n, cw)
            ref = np.array([(cw + i) // n for i in range(n)]).astype(np.int32)
            assert got.dtype == np.int32 and np.array_equal(got, ref)
            assert int(got.sum()) == cw


# ------------------------------------------------------------------------------ the atlas on the host

def test_render_equals_direct_pil_drawing():
    PIL = pytest.importorskip("PIL")  # noqa: F841
    from PIL import Image, ImageDraw, ImageFont
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    font = ImageFont.load_default()
    symbols = {ch: i + 1 for i, ch in enumerate("AbgQ#7 ~")}
    for fs, bg, fg in ((24, (255, 255, 255), (0, 0, 0)), (16, (200, 200, 200), (40, 40, 40))):
        atlas = GlyphAtlas.render(symbols, font, fs, bg, fg, cell=102, stride=3)
        assert atlas.glyphs.shape == (len(symbols) + 1, fs, fs) and atlas.glyphs.dtype == np.uint8
        assert (atlas.cell, atlas.stride, atlas.margin, atlas.src_w, atlas.height) == (102, 3, 102, fs, fs)
        assert (atlas.glyphs[0] == bg[0]).all(), "PAD is background"
        for ch, i in symbols.items():
            im = Image.new("RGB", (fs, fs), bg)
            ImageDraw.Draw(im).text((0, 0), ch, fill=fg, font=font)
            assert np.array_equal(atlas.glyphs[i], np.asarray(im.convert("L"))), ch
        assert (atlas.glyphs[symbols["A"]] != bg[0]).any(), "ink was drawn"
    seq = GlyphAtlas.render("Ab", font, 24)  # a sequence: ids from 1; the cell defaults to the font size
    assert seq.glyphs.shape == (3, 24, 24) and seq.cell == 24 and seq.stride == 1
    assert np.array_equal(seq.glyphs[1], GlyphAtlas.render({"A": 1}, font, 24).glyphs[1])
    for bad in dict(background=(255, 255, 254)), dict(text=(0, 1, 0)), dict(text=(0, 0)), dict(background=(256,) * 3):
        with pytest.raises(ValueError, match="not gray"):
            GlyphAtlas.render(symbols, font, 24, **bad)
    with pytest.raises(ValueError, match="start at 1"):
        GlyphAtlas.render({"A": 0}, font, 24)


def test_from_config_reads_the_packaged_metadata():
    pytest.importorskip("PIL")
    from PIL import ImageFont
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    from visual_onoma_to_wave_amd.utils.symbols import get_symbols
    pc = configs()[0]
    atlas = GlyphAtlas.from_config(pc, font=ImageFont.load_default())
    syms = get_symbols(pc["path"]["preprocessed"])
    assert atlas.glyphs.shape == (len(syms) + 1, 24, 24) and (atlas.cell, atlas.stride) == (102, 1)


def test_host_validation():
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    g = C.random_glyphs(0, 4, 24, 24)
    for bad in (g.astype(np.int32), g[0], g[:0]):
        with pytest.raises(ValueError, match="glyphs must be uint8"):
            GlyphAtlas(bad, 102)
    for cell, stride in ((0, 1), (102, 0)):
        with pytest.raises(ValueError, match="must be >= 1"):
            GlyphAtlas(g, cell, stride)
    atlas = GlyphAtlas(g, 102, 3)
    assert (atlas.n_symbols, atlas.height, atlas.src_w, atlas.margin) == (4, 24, 24, 102)
    with pytest.raises(RuntimeError, match="to\\(device\\) first"):
        atlas.layout(np.zeros((1, 2), np.int64), [2])
    # the checks themselves need no device: a CPU "device" holds the tensors, and every refusal precedes the launch
    atlas.to("cpu")
    ids = np.array([[1, 2, 3], [3, 0, 0]])
    for bad in (np.array([[1, 2, 4]]), np.array([[-1, 0, 0]])):
        with pytest.raises(ValueError, match="texts must be in \\[0, 3\\]"):
            atlas.layout(bad, [3])
    for bad in ([[103, 1, 1], [1, 1, 1]], [[-1, 1, 1], [1, 1, 1]]):
        with pytest.raises(ValueError, match="widths must be in \\[0, 102\\]"):
            atlas.layout(ids, [3, 1], np.array(bad))
    with pytest.raises(ValueError, match="must be integers"):
        atlas.layout(ids, [3, 1], np.ones((2, 3)))
    with pytest.raises(ValueError, match="texts must have shape"):
        atlas.layout(ids[0], [3])
    with pytest.raises(ValueError, match="n_chars=2 is below"):
        atlas.layout(ids, [3, 1], n_chars=2)
    with pytest.raises(RuntimeError, match="GPU only"):  # valid arguments reach the launch, which has no CPU form
        atlas.layout(ids, [3, 1], np.array([[0, 24, 102], [1, 1, 1]]))
