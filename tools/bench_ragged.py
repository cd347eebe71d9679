#!/usr/bin/env python
"""Dense against ragged ``Generator.run`` at the headline vocoder shape (B = 32 x 512 mel frames, bf16).

Lengths are uniform in [128, 512] from a fixed seed; the same padded batch runs dense (every frame computed) and
ragged (``lengths`` given: DESIGN.md section 10).  Each variant is timed with device events over blocks of whole
runs, the two alternating, after a warm-up; every block lasts at least ``--window`` seconds.  Then one pass of each
under the profiling timer gives the MRF stages' times (tags mrf_s0 .. mrf_s3) and how close each ragged stage comes to
fill = sum(len) / (B T) of its dense time.  Prints one JSON line.

    python tools/bench_ragged.py [--batch 32] [--frames 512] [--blocks 5] [--window 0.5]
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--min-frames", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per variant (alternating)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed block, at least")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()

    from visual_onoma_to_wave_amd import hifigan, synth
    from visual_onoma_to_wave_amd.profiling import KernelTimer
    data = os.path.join(os.path.dirname(os.path.abspath(hifigan.__file__)), "..", "data")
    with open(os.path.join(data, "hifigan_config.json")) as f:
        h = hifigan.AttrDict(json.load(f))
    torch.manual_seed(a.seed)
    gen = hifigan.Generator(h)
    gen.eval()
    gen.remove_weight_norm()
    gen = gen.cuda()
    gen.set_compute_dtype(torch.bfloat16)

    rng = np.random.default_rng(a.seed)
    B, T = a.batch, a.frames
    mel = torch.from_numpy(synth.mels(rng, B, T, channels_last=True)).cuda()
    lens_h = rng.integers(a.min_frames, T + 1, size=B)
    for b in range(B):  # padded as vTTS pads
        mel[b, int(lens_h[b]):] = 0.0
    lens = torch.from_numpy(lens_h.astype(np.int64)).cuda()
    fill = float(lens_h.sum()) / (B * T)

    variants = {"dense": lambda: gen.run(mel), "ragged": lambda: gen.run(mel, lens)}
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()

        def block(fn, n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                fn()
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / n
        n = max(3, int(a.window * 1000.0 / block(variants["dense"], 5)) + 1)  # dense runs per window; ragged ones are shorter
        times = {k: [] for k in variants}
        for _ in range(a.blocks):
            for k, fn in variants.items():
                m = n
                t = block(fn, m)
                while t * m < a.window * 1000.0:  # a faster variant: more runs, until the block fills the window
                    m *= 2
                    t = block(fn, m)
                times[k].append(t)
        stages = {}
        for k, fn in variants.items():
            with KernelTimer([f"mrf_s{i}" for i in range(4)]) as timer:
                for _ in range(10):
                    fn()
                summ = timer.summary()
            stages[k] = {tag: d["total_ms"] / 10 for tag, d in sorted(summ.items())}

    med = {k: statistics.median(v) for k, v in times.items()}
    out = dict(shape=[B, T], fill=round(fill, 4), runs_per_block=n,
               dense_ms=[round(t, 4) for t in times["dense"]], ragged_ms=[round(t, 4) for t in times["ragged"]],
               dense_median_ms=round(med["dense"], 4), ragged_median_ms=round(med["ragged"], 4),
               dense_spread_ms=round(max(times["dense"]) - min(times["dense"]), 4),
               ragged_over_dense=round(med["ragged"] / med["dense"], 4),
               stage_ms={k: {t: round(v, 4) for t, v in s.items()} for k, s in stages.items()},
               stage_ragged_over_dense={t: round(stages["ragged"][t] / stages["dense"][t], 4) for t in stages["dense"]})
    print(json.dumps(out))
    ok = med["ragged"] <= med["dense"] + (max(times["dense"]) - min(times["dense"]))
    print(f"fill {fill:.3f}; ragged / dense {med['ragged'] / med['dense']:.3f}; "
          f"{'ragged is not slower than dense' if ok else 'RAGGED IS SLOWER THAN DENSE beyond the run-to-run spread'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
