"""The yardstick of glyph stretching: PIL's bicubic resample, horizontal pass only, restated
with Python floats (IEEE double, one rounding per operation) and int32 numpy sums, and the layout of
``vo_glyph_stretch`` on top of it.  tests/test_glyph_stretch_cpu.py pins this model against Pillow itself and the
library's table against this model; the GPU tests compare the kernel with ``layout``.

The rule, for source width S and target width w >= 1 (PIL: precompute_coeffs, bicubic_filter,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc):

    scale = S / w;  fs = max(scale, 1.0);  support = 2.0 * fs;  ss = 1.0 / fs
    column c:  center = (c + 0.5) * scale
               xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), S);  n = xmax - xmin
               k[x] = bicubic((x + xmin - center + 0.5) * ss);  k[x] /= sum(k) (in index order, when it is not 0)
               K[x] = int(k[x] * 2^22 + 0.5) for k[x] >= 0, int(k[x] * 2^22 - 0.5) below (truncation toward 0)
    pixel:     clamp((2^21 + sum_x src[y][xmin + x] * K[x]) >> 22, 0, 255)
"""

import functools

import numpy as np

BITS = 22
GEOMETRIES = ((24, 102), (16, 40), (32, 64))  # (S, cell): the packaged glyph, and two that share neither number


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def record(S, w, c):
    """(xmin, n, K (n,) Python ints) of output column c at target width w."""
    scale = float(S) / w
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    center = (c + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), S)
    n = xmax - xmin
    k = [bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
    ww = 0.0
    for v in k:
        ww += v
    if ww != 0.0:
        k = [v / ww for v in k]
    K = [int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in k]
    return xmin, n, K


@functools.lru_cache(maxsize=None)
def table(S, cell):
    """The table of ``vo_glyph_stretch_table``: (cell (cell + 1) / 2, 2 + S) int32, record w (w - 1) / 2 + c =
    xmin, n, K[0 .. S) with zeros past n.  Read-only (shared between tests)."""
    out = np.zeros((cell * (cell + 1) // 2, 2 + S), np.int32)
    for w in range(1, cell + 1):
        for c in range(w):
            xmin, n, K = record(S, w, c)
            r = out[w * (w - 1) // 2 + c]
            r[0], r[1] = xmin, n
            r[2:2 + n] = K
    out.setflags(write=False)
    return out


def resize(glyph, w, tab=None):
    """glyph (H, S) uint8 -> (H, w) uint8."""
    glyph = np.asarray(glyph, np.uint8)
    H, S = glyph.shape
    if tab is None:
        tab = table(S, max(w, S))
    out = np.empty((H, w), np.uint8)
    src = glyph.astype(np.int32)
    for c in range(w):
        r = tab[w * (w - 1) // 2 + c]
        xmin, n = int(r[0]), int(r[1])
        acc = np.int32(1 << (BITS - 1)) + (src[:, xmin:xmin + n] * r[2:2 + n][None, :]).sum(axis=1, dtype=np.int32)
        out[:, c] = np.clip(acc >> BITS, 0, 255)
    return out


def acc_bound(tab):
    """The largest |2^21 + sum_x src[x] K[x]| any source row in [0, 255] gives, over every record of ``tab``."""
    K = tab[:, 2:].astype(np.int64)
    hi = (1 << (BITS - 1)) + 255 * np.where(K > 0, K, 0).sum(axis=1)
    lo = (1 << (BITS - 1)) + 255 * np.where(K < 0, K, 0).sum(axis=1)
    return int(max(hi.max(), -lo.min()))


def layout(atlas, ids, src_lens, widths, cell, margin, W_out=None):
    """What ``vo_glyph_stretch`` writes: (B, 1, H, W_out) float32.  atlas (n, H, S) uint8, ids (B, T), src_lens (B,),
    widths (B, T) or None (every width S)."""
    atlas = np.asarray(atlas, np.uint8)
    n_glyphs, H, S = atlas.shape
    ids = np.asarray(ids)
    B, T = ids.shape
    if W_out is None:
        W_out = T * cell + 2 * margin
    assert W_out >= T * cell + 2 * margin
    tab = table(S, cell)
    img = np.full((B, H, W_out), 255, np.uint8)
    for b in range(B):
        for t in range(T):
            wr = S if widths is None else int(widths[b][t])
            i = int(ids[b][t])
            if t >= int(src_lens[b]) or wr <= 0 or not 0 <= i < n_glyphs:
                continue
            w = min(wr, cell)
            pleft = (cell - w) // 2 + (cell - w) % 2
            x0 = margin + t * cell + pleft
            img[b, :, x0:x0 + w] = resize(atlas[i], w, tab)
    return (img.astype(np.float32) / np.float32(255.0))[:, None]


def random_glyphs(seed, n, H, S, binary=False):
    """n seeded glyphs (n, H, S) uint8: random gray, or black on white."""
    rng = np.random.default_rng(seed)
    if binary:
        return np.where(rng.random((n, H, S)) < 0.4, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, size=(n, H, S), dtype=np.uint8)


def pil_resize(glyph, w):
    """The reference's three calls on a gray RGB image holding ``glyph``: resize((w, H)), no filter argument, then
    convert("L") (visualtext_generator.py:36-39, dataset's / prediction.ipynb's convert)."""
    from PIL import Image
    g = np.asarray(glyph, np.uint8)
    im = Image.fromarray(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)))  # (H, S, 3) uint8: mode RGB
    return np.asarray(im.resize((int(w), g.shape[0])).convert("L"), dtype=np.uint8)
