"""Latency of one synthesis request batch, eager against graphed.

What is timed: a host clock (perf_counter) from "request tensors on the device" to "int16 arrays on the host",
ending in a device synchronise.
  A (eager):   model(..., max_mel_len=cap) -> vocoder.run(out[1], out[9], pcm_scale) -> copy wav and mel_len to the
               host, cut per utterance
  B (graphed): pipeline.GraphedSynthesis(...)(...) -> res.wavs()
Shapes (B, T_src, cap): (1, 4, 64), (8, 12, 256), (32, 12, 512).  Synthetic weights with the duration predictor's
output bias shifted by +1.6 (as the tests: without it the predicted lengths are zero), mixed precision, bf16 vocoder.
Protocol: both paths warmed, then blocks of A and B alternate in one process (A B A B ...), --blocks blocks of
--block requests per path and shape (default 4 x 60 = 240 requests per path).  Reported per path: median and p90 over
all requests, and the spread = the largest difference between the medians of two blocks of the same path -- a
difference of the medians of A and B that is not larger than that spread is not a result.

    python tools/latency_ab.py --out profiles/graphed/latency.json
"""

import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # before the HIP runtime initialises (train.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((1, 4, 64), (8, 12, 256), (32, 12, 512))
PCM_SCALE = 32768.0
DUR_BIAS_SHIFT = 1.6
HOP = 256


def build(dev):
    from helpers import configs, hifigan_arrays, hifigan_h, vtts_arrays
    from weights import load_into
    from visual_onoma_to_wave_amd import hifigan
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    m = m.to(dev).eval().set_precision("mixed")
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.linear_layer.bias += DUR_BIAS_SHIFT
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    g = g.to(dev)
    g.set_compute_dtype(torch.bfloat16)
    return m, g


def requests(dev, B, T_src, k=4):
    """k request batches on the device (the timed paths cycle through them)."""
    from visual_onoma_to_wave_amd import synth
    out = []
    for s in range(k):
        b = synth.acoustic_batch(9000 + s, B, T_src, 20, ragged=B > 1)
        out.append({n: torch.from_numpy(b[n]).to(dev) for n in ("audiotypes", "texts", "src_lens", "images")})
    return out


def eager(m, g, q, T_src, cap):
    with torch.no_grad():
        out = m(q["audiotypes"], q["texts"], q["src_lens"], T_src, None, None, cap, None, None, None, q["images"],
                None, True)
        wav = g.run(out[1], out[9], PCM_SCALE)
    wav = wav.cpu().numpy()
    n = np.minimum(out[9].cpu().numpy(), cap) * HOP
    torch.cuda.synchronize()
    return [wav[i, :int(n[i])] for i in range(wav.shape[0])]


def graphed(gs, q):
    w = gs(q["audiotypes"], q["src_lens"], q["images"], texts=q["texts"]).wavs()
    torch.cuda.synchronize()
    return w


def timed(fn, reqs, n):
    ts = []
    for i in range(n):
        q = reqs[i % len(reqs)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(q)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(blocks):
    allt = np.concatenate(blocks)
    meds = [float(np.median(b)) for b in blocks]
    return dict(median_ms=float(np.median(allt)), p90_ms=float(np.percentile(allt, 90)), n=int(allt.size),
                block_medians_ms=meds, spread_ms=float(max(meds) - min(meds)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.blocks * a.block < 200:
        ap.error("at least 200 requests per path and shape")
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    dev = torch.device("cuda:0")
    m, g = build(dev)
    result = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                  pcm_scale=PCM_SCALE, blocks=a.blocks, block=a.block,
                  clock="host perf_counter, request tensors on the device -> int16 arrays on the host + synchronise",
                  shapes=[])
    for B, T_src, cap in SHAPES:
        reqs = requests(dev, B, T_src)
        gs = GraphedSynthesis(m, g, B, T_src, cap, pcm_scale=PCM_SCALE)
        fa = lambda q: eager(m, g, q, T_src, cap)  # noqa: E731
        fb = lambda q: graphed(gs, q)  # noqa: E731
        for q in reqs:  # the two paths give the same samples
            for x, y in zip(fa(q), fb(q)):
                np.testing.assert_array_equal(x, y)
        timed(fa, reqs, a.warmup), timed(fb, reqs, a.warmup)
        A, Bk = [], []
        for _ in range(a.blocks):
            A.append(timed(fa, reqs, a.block))
            Bk.append(timed(fb, reqs, a.block))
        sa, sb = summary(A), summary(Bk)
        secs = [float(len(w)) / 22050 for w in fb(reqs[0])]
        gain = sa["median_ms"] - sb["median_ms"]
        row = dict(B=B, T_src=T_src, cap=cap, mean_audio_s=float(np.mean(secs)), eager=sa, graphed=sb,
                   median_gain_ms=gain, gain_exceeds_spread=bool(gain > max(sa["spread_ms"], sb["spread_ms"])),
                   captures=gs.captures)
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
