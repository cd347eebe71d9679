"""Golden vector for glyph stretching, from Pillow's own resize and the oracle's layout.

The reference renders a character with three PIL calls and stretches it with a fourth
(scripts/preprocessor/visualtext_generator.py:36-40):

    c_im = Image.new("RGB", (fontsize, fontsize), bgcolor)
    draw = ImageDraw.Draw(c_im);  draw.text((0, 0), char, fill=txtcolor, font=font)
    c_im = c_im.resize((width, fontsize))
    canvas.paste(c_im, (w, 0))

and its loaders read the strip back as gray (``convert("L")``).  This script makes the same calls per character with
ONE substitution: there is no font file where the goldens are made, so ``draw.text`` is replaced by pasting a seeded
synthetic bitmap (gray in all three channels, as black text on white is) into ``c_im``.  What is pinned is the resize
and the layout, not a rasteriser.  The strips and their widths then go through ``oracle.data.glyph_batch`` (the
reference's character_padding_forinput + pad_2D_gray_image + ToTensor).  Written, as data only:

    glyph_stretch.npz   glyphs (12, 24, 24) uint8 (row 0: PAD, white), ids (7, 17) int64, widths (7, 17) int32,
                        lens (7,) int64, cell, stride, expected (7, 1, 24, 17 * 102 + 2 * 102) float32

The 102 characters of the 7 rows (17, 17, 17, 17, 17, 12 and 5 of them) carry every width 1 .. 102 once, in a seeded
order; ids and widths are 0 past a row's length.  Needs Pillow, not the reference's tree.

    python tests/golden/make_goldens_stretch.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

FS, CELL, STRIDE, T = 24, 102, 3, 17
LENS = (17, 17, 17, 17, 17, 12, 5)
N_GLYPHS = 12
BG = (255, 255, 255)


def synthetic_glyphs(rng):
    """Black strokes on white: a random 6 x 6 pattern at 4 px per dot, every other glyph with its edges softened to
    grays by a 3-tap horizontal mean (an antialiased rasteriser gives such edges)."""
    glyphs = np.full((N_GLYPHS, FS, FS), 255, np.uint8)
    for i in range(1, N_GLYPHS):
        dots = rng.random((6, 6)) < 0.4
        g = np.where(np.kron(dots, np.ones((4, 4), bool)), 0, 255).astype(np.int32)
        if i % 2:
            p = np.pad(g, ((0, 0), (1, 1)), mode="edge")
            g = (p[:, :-2] + p[:, 1:-1] + p[:, 2:]) // 3
        glyphs[i] = g.astype(np.uint8)
    return glyphs


def draw(glyphs, ids, widths):
    """One text as the reference's Generator.draw draws it in stretching mode -> (strip (FS, sum widths) uint8)."""
    from PIL import Image
    canvas = Image.new("RGB", (int(sum(widths)), FS), BG)
    w = 0
    for i, width in zip(ids, widths):
        c_im = Image.new("RGB", (FS, FS), BG)
        c_im.paste(Image.fromarray(np.ascontiguousarray(np.repeat(glyphs[i][:, :, None], 3, axis=2))), (0, 0))
        c_im = c_im.resize((int(width), FS))
        canvas.paste(c_im, (w, 0))
        w += int(width)
    return np.asarray(canvas.convert("L"), dtype=np.uint8)


def main():
    from oracle import data as O
    rng = np.random.default_rng(2409)
    glyphs = synthetic_glyphs(rng)
    all_widths = rng.permutation(np.arange(1, CELL + 1))
    assert sum(LENS) == CELL
    B = len(LENS)
    ids = np.zeros((B, T), np.int64)
    widths = np.zeros((B, T), np.int32)
    strips, char_widths, k = [], [], 0
    for b, n in enumerate(LENS):
        ids[b, :n] = rng.integers(1, N_GLYPHS, size=n)
        widths[b, :n] = all_widths[k:k + n]
        k += n
        strips.append(draw(glyphs, ids[b, :n], widths[b, :n]))
        char_widths.append(widths[b, :n])
    expected = O.glyph_batch(strips, char_widths, CELL, STRIDE)
    assert expected.shape == (B, 1, FS, T * CELL + 2 * (STRIDE // 2) * CELL) and expected.dtype == np.float32
    path = os.path.join(HERE, "glyph_stretch.npz")
    np.savez_compressed(path, glyphs=glyphs, ids=ids, widths=widths, lens=np.asarray(LENS, np.int64),
                        cell=np.int64(CELL), stride=np.int64(STRIDE), expected=expected)
    print("wrote", os.path.relpath(path, REPO), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
