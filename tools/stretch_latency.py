"""Latency of one synthesis request batch after a change of character widths.

What is timed: a host clock (perf_counter) from "the request is known" to "int16 arrays on the host", ending in a
device synchronise, through ``pipeline.GraphedSynthesis`` in every arm:
  a (images):  the images already on the device (drawn before the clock starts) -> gs(images=...) -> res.wavs().
               The path without an atlas, as before: it cannot follow a width change by itself.
  b (pil):     the widths on the host -> PIL ``resize`` per character (the notebook's loop), the strips pasted ->
               ``GlyphBatch.to(device, n_chars)`` -> gs(images=...) -> res.wavs().  What a user of the image path pays
               after a width change.
  c (atlas):   the widths already on the device -> gs(texts=..., widths=...) with an atlas -> res.wavs(): the glyphs
               are stretched by the graph's first launch.  The counterpart of a.
  d (atlas, host widths): as c with the widths a host array (validated, one small upload).  The counterpart of b.
Shapes (B, T_src, cap): (1, 4, 64), (8, 12, 256), (32, 12, 512); model, weights and precisions as tools/latency_ab.py;
seeded black-on-white 24 x 24 glyphs for the 73 symbols, widths uniform in 6 .. 102.  All arms give the same samples
(asserted before timing).
Protocol: every arm warmed, then blocks of a, b, c, d alternate in one process, --blocks blocks of --block requests
per arm and shape.  Reported per arm: median and p90 over all requests, and the spread = the largest difference
between the medians of two blocks of the same arm.  ``c_minus_a_ms`` against ``max(spread a, spread c)`` is the check
that the atlas costs nothing; ``b_minus_d_ms`` is what a user gains.

    python tools/stretch_latency.py --out profiles/stretch/latency.json
"""

import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # before the HIP runtime initialises (train.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import latency_ab as LA  # noqa: E402

FS, CELL = 24, 102


def make_atlas(dev):
    from visual_onoma_to_wave_amd.dataset import GlyphAtlas
    rng = np.random.default_rng(73)
    glyphs = np.where(rng.random((73, FS, FS)) < 0.3, 0, 255).astype(np.uint8)
    glyphs[0] = 255
    return GlyphAtlas(glyphs, CELL, 1).to(dev)


def requests(dev, atlas, B, T_src, k=4):
    """k request batches: ids, lengths and widths on the host and on the device, and the images of arm a."""
    from visual_onoma_to_wave_amd import synth
    out = []
    for s in range(k):
        b = synth.acoustic_batch(9100 + s, B, T_src, 20, ragged=B > 1)
        widths = np.random.default_rng(s).integers(6, CELL + 1, size=(B, T_src)).astype(np.int32)
        q = {n: torch.from_numpy(b[n]).to(dev) for n in ("audiotypes", "texts", "src_lens")}
        q.update(texts_h=b["texts"], src_lens_h=b["src_lens"], widths_h=widths,
                 widths=torch.from_numpy(widths).to(dev))
        q["images"] = atlas.layout(q["texts"], q["src_lens"], q["widths"], n_chars=T_src)
        out.append(q)
    return out


def pil_images(atlas, q, dev, T_src):
    """The notebook's loop: every character resized by PIL and pasted, then the batch laid out on the device."""
    from PIL import Image
    from visual_onoma_to_wave_amd.dataset import GlyphBatch
    strips, cw = [], []
    for b in range(len(q["src_lens_h"])):
        n = int(q["src_lens_h"][b])
        canvas = Image.new("L", (int(q["widths_h"][b, :n].sum()), FS), 255)
        x = 0
        for t in range(n):
            w = int(q["widths_h"][b, t])
            canvas.paste(Image.fromarray(atlas.glyphs[q["texts_h"][b, t]]).resize((w, FS)), (x, 0))
            x += w
        strips.append(np.asarray(canvas, dtype=np.uint8))
        cw.append(q["widths_h"][b, :n])
    return GlyphBatch(strips, cw, CELL, 1).to(dev, n_chars=T_src)


def kernels(dev, n):
    """``--kernels N``: N launches each of glyph_stretch_kernel and glyph_batch_kernel writing the same
    (32, 1, 24, 12 * 102) output, and nothing else -- for a ``rocprofv3 --kernel-trace --stats`` run of their own."""
    atlas = make_atlas(dev)
    q = requests(dev, atlas, 32, 12, k=1)[0]
    from visual_onoma_to_wave_amd import ops
    from visual_onoma_to_wave_amd.dataset import GlyphBatch
    strips = [np.concatenate([np.full((FS, int(w)), 128, np.uint8) for w in q["widths_h"][b]], axis=1)
              for b in range(32)]
    batch = GlyphBatch(strips, list(q["widths_h"]), CELL, 1)
    full = torch.full((32,), 12, dtype=torch.int64, device=dev)
    out = torch.empty((32, 1, FS, 12 * CELL), device=dev)
    for _ in range(n):
        ops.glyph_stretch(atlas.glyphs_d, atlas.table_d, q["texts"], full, q["widths"], CELL, 0, out=out)
        batch.to(dev, n_chars=12)
    torch.cuda.synchronize()
    print(f"{n} launches of each kernel, output {tuple(out.shape)} fp32 = {out.numel() * 4} bytes")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernels", type=int, default=0, help="only launch the two layout kernels N times (for a trace)")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels:
        return kernels(torch.device("cuda:0"), a.kernels)
    if a.blocks * a.block < 200:
        ap.error("at least 200 requests per arm and shape")
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    dev = torch.device("cuda:0")
    m, g = LA.build(dev)
    atlas = make_atlas(dev)
    result = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                  pcm_scale=LA.PCM_SCALE, blocks=a.blocks, block=a.block,
                  clock="host perf_counter, request known -> int16 arrays on the host + synchronise", shapes=[])
    for B, T_src, cap in LA.SHAPES:
        reqs = requests(dev, atlas, B, T_src)
        gs_i = GraphedSynthesis(m, g, B, T_src, cap, pcm_scale=LA.PCM_SCALE)
        gs_a = GraphedSynthesis(m, g, B, T_src, cap, pcm_scale=LA.PCM_SCALE, atlas=atlas)

        def sync(res):
            w = res.wavs()
            torch.cuda.synchronize()
            return w

        arms = dict(
            a_images=lambda q: sync(gs_i(q["audiotypes"], q["src_lens"], q["images"], texts=q["texts"])),
            b_pil=lambda q: sync(gs_i(q["audiotypes"], q["src_lens"], pil_images(atlas, q, dev, T_src),
                                      texts=q["texts"])),
            c_atlas=lambda q: sync(gs_a(q["audiotypes"], q["src_lens"], texts=q["texts"], widths=q["widths"])),
            d_atlas_host_widths=lambda q: sync(gs_a(q["audiotypes"], q["src_lens"], texts=q["texts"],
                                                    widths=q["widths_h"])))
        for q in reqs:  # every arm gives the same samples
            ref = arms["a_images"](q)
            for name in ("b_pil", "c_atlas", "d_atlas_host_widths"):
                for x, y in zip(ref, arms[name](q)):
                    np.testing.assert_array_equal(x, y, err_msg=name)
        for fn in arms.values():
            LA.timed(fn, reqs, a.warmup)
        blocks = {name: [] for name in arms}
        for _ in range(a.blocks):
            for name, fn in arms.items():
                blocks[name].append(LA.timed(fn, reqs, a.block))
        s = {name: LA.summary(v) for name, v in blocks.items()}
        c_minus_a = s["c_atlas"]["median_ms"] - s["a_images"]["median_ms"]
        spread = max(s["a_images"]["spread_ms"], s["c_atlas"]["spread_ms"])
        row = dict(B=B, T_src=T_src, cap=cap, **s, c_minus_a_ms=c_minus_a, spread_a_c_ms=spread,
                   c_within_spread_of_a=bool(c_minus_a <= spread),
                   b_minus_d_ms=s["b_pil"]["median_ms"] - s["d_atlas_host_widths"]["median_ms"],
                   captures=[gs_i.captures, gs_a.captures])
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
