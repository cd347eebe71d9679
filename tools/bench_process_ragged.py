#!/usr/bin/env python
"""``FeatureExtractor.process`` on a corpus-like batch: 64 synthetic utterances of 64 distinct lengths between 0.2 s
and 3 s (22.05 kHz), eight characters each.  Nearly every clip of a real corpus has its own length; before the ragged
mel front end such a call made one launch pair and three small copies per utterance.

One tree (the repository this script lies in, or ``--root DIR``: a checkout whose package is built) per process:
warm-up calls, then ``--blocks`` timed blocks of at least ``--window`` seconds each, the host clock around calls that
end in their device-to-host copies and a device synchronise.  Prints one JSON line: ms per call of each block and the
SHA-256 of every result's bytes (the same inputs must give the same features in every tree).

    python tools/bench_process_ragged.py [--root DIR]
    python tools/bench_process_ragged.py --compare parent=DIR tree=DIR [--rounds 3] --out FILE.json

``--compare`` runs the trees in child processes, alternating, and writes the comparison.
"""

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SR, N_UTT, N_CHARS = 22050, 64, 8


def corpus(seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = np.linspace(0.2 * SR, 3.0 * SR, N_UTT).astype(int) + rng.integers(0, 200, N_UTT)
    assert len(set(lens.tolist())) == N_UTT
    lens = lens[rng.permutation(N_UTT)]
    wavs, durs = [], []
    for n in lens:
        t = np.arange(n) / SR
        w = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
                for f in rng.uniform(80, 7000, size=4)) + 0.01 * rng.standard_normal(n)
        wavs.append(w.astype(np.float32))
        F = 1 + n // 256
        cuts = np.sort(rng.integers(0, F, N_CHARS - 1))  # eight spans covering F - 1 frames, some possibly empty
        durs.append(np.diff(np.concatenate([[0], cuts, [F - 1]])).astype(int))
    return wavs, durs


def run_one(a):
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.dirname(HERE))
    import torch
    import yaml
    import visual_onoma_to_wave_amd as pkg
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    if not torch.cuda.is_available():
        raise SystemExit("bench_process_ragged: needs a GPU (a CPU timing says nothing)")
    with open(os.path.join(os.path.dirname(pkg.__file__), "data", "config", "ICASSP", "preprocess.yaml")) as f:
        fx = FeatureExtractor(yaml.safe_load(f))
    wavs, durs = corpus(a.seed)

    def call():
        out = fx.process(wavs, durs)
        torch.cuda.synchronize()
        return out
    for _ in range(a.warmup):
        out = call()
    h = hashlib.sha256()
    for o in out:
        for k in ("mel", "energy", "kurtosis"):
            h.update(o[k].tobytes())
    t0 = time.perf_counter()
    call()
    n = max(3, int(a.window / (time.perf_counter() - t0)) + 1)
    ms = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        ms.append((time.perf_counter() - t0) * 1000.0 / n)
    print(json.dumps(dict(root=os.path.dirname(os.path.dirname(pkg.__file__)), utterances=N_UTT,
                          samples=int(sum(len(w) for w in wavs)), calls_per_block=n,
                          ms_per_call=[round(t, 4) for t in ms], median_ms=round(statistics.median(ms), 4),
                          results_sha256=h.hexdigest())))
    return 0


def compare(a):
    trees = [s.split("=", 1) for s in a.compare]
    res = {k: dict(ms_per_call=[], results_sha256=[]) for k, _ in trees}
    for r in range(a.rounds):
        for k, root in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--seed", str(a.seed),
                                "--blocks", str(a.blocks), "--window", str(a.window), "--warmup", str(a.warmup)],
                               check=True, capture_output=True, text=True, timeout=a.child_timeout)
            d = json.loads(p.stdout.strip().splitlines()[-1])
            res[k]["ms_per_call"].append(d["median_ms"])
            res[k]["results_sha256"].append(d["results_sha256"])
            print(k, r + 1, d, flush=True)
    shas = {s for v in res.values() for s in v["results_sha256"]}
    out = dict(command="tools/bench_process_ragged.py --compare " + " ".join(k + "=DIR" for k, _ in trees),
               workload=f"FeatureExtractor.process, {N_UTT} utterances of {N_UTT} distinct lengths in [0.2 s, 3 s], "
                        f"{N_CHARS} characters each, fp32",
               order="one process per run on one MI355X, alternating " + ", ".join(k for k, _ in trees) +
                     f", {a.rounds} rounds; per run the median of {a.blocks} blocks of >= {a.window} s",
               **{k: dict(median_ms_per_call=v["ms_per_call"], results_sha256=v["results_sha256"])
                  for k, v in res.items()},
               results_identical_in_all_runs=len(shas) == 1)
    k0, k1 = trees[0][0], trees[-1][0]
    out[f"{k1}_over_{k0}"] = round(statistics.median(res[k1]["ms_per_call"]) /
                                   statistics.median(res[k0]["ms_per_call"]), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", help="checkout to measure (default: this script's)")
    ap.add_argument("--compare", nargs="+", metavar="NAME=DIR")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="process_parent_vs_tree.json")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed block, at least")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=64)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    return compare(a) if a.compare else run_one(a)


if __name__ == "__main__":
    sys.exit(main())
