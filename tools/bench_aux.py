#!/usr/bin/env python3
"""Measurement of the SURVEY.md 8(f) rows 2-3 on one MI355X (one JSON line each):

* glyph batch (vo_glyph_batch): a C4 training batch of 48 utterances (12 x group 4) of up to 21
  characters, 24 x 102 px cells -> (B, 1, 24, W) fp32; HBM roofline on the algorithmic bytes
  (uint8 strips in + fp32 out); CPU baseline = the reference's numpy layout (oracle/data.py).
* feature extraction (vo_stft_mel_ex + vo_char_features): 64 utterances of 2 s at 22.05 kHz
  -> mel + character energy + kurtosis; CPU baseline = oracle/mel.char_features (torch-CPU).

* augmented batch (vo_augment_batch, dataset.DeviceCorpus): a training batch of 48 mixed repeat / consecutive
  variants from a synthetic corpus of ICASSP-like sizes, assembled on the device from a device plan, against the
  path it replaces: the variants' files materialised in a temporary directory, read through Dataset.__getitem__,
  collate_fn and to_device.  Bytes per second are the batch's output bytes over the launch time.

* corpus statistics (vo_corpus_stats): the energy statistics of the reference's feature normalisation over every row
  of that corpus's variant plan, against numpy over the materialised arrays.

* vocoder training batch (vo_segment_plan + vo_segment_batch, hifigan.data.SegmentSampler): 16 segments of 8192
  samples and their mel frames drawn and cut on the device from that corpus with int16 waveforms attached, against
  numpy crops of the same rows and their upload.  ``segments-c5`` (only when named): the C5 training step replayed
  with the batch drawn inside the graph against the replay over static tensors.

* sample-rate conversion (vo_resample): 64 rows of 2 s of int16 PCM at 48 kHz -> fp32 at 22.05 kHz in one launch,
  the achieved fp32 rate beside the vector peak and the byte bound, and the upload of the same batch for scale.

    python tools/bench_aux.py [glyph] [features] [augment] [stats] [segments] [resample] [--out FILE]   (these six by default)
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_aux.py augment --kernels 200   (launches only)
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0
FP32_VECTOR_PEAK_TFLOPS = 157.3  # the spec figure: packed FMA on every lane; a scalar-FMA loop can reach half of it


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n / 1e3


def glyph():
    from oracle import data as O
    from visual_onoma_to_wave_amd import ops
    rng = np.random.default_rng(0)
    B, H, cell = 48, 24, 102
    widths = [rng.integers(30, cell + 1, int(rng.integers(4, 22))) for _ in range(B)]
    strips = [rng.integers(0, 256, (H, int(w.sum()))).astype(np.uint8) for w in widths]
    dev = torch.device("cuda")
    # device-resident strips: time the layout kernel itself (the host packs / uploads once per batch)
    out = ops.glyph_batch(strips, widths, cell, 0, dev)
    n_in = sum(s.size for s in strips)
    t_e2e = timed(lambda: ops.glyph_batch(strips, widths, cell, 0, dev), 20)  # incl. pack + H2D
    # kernel only: replay with pre-uploaded buffers through the C ABI
    import ctypes
    from visual_onoma_to_wave_amd import _lib
    offs = np.zeros(B, np.int64)
    offs[1:] = np.cumsum([s.size for s in strips])[:-1]
    cw = np.concatenate(widths).astype(np.int32)
    co = np.zeros(B + 1, np.int32)
    co[1:] = np.cumsum([len(w) for w in widths])
    cs = np.concatenate([np.concatenate([[0], np.cumsum(w)[:-1]]) for w in widths]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    px, of, iw, cod, csd, cwd = (t(np.concatenate([s.reshape(-1) for s in strips])), t(offs),
                                 t(np.array([s.shape[1] for s in strips], np.int32)), t(co), t(cs), t(cw))
    W = out.shape[-1]
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def k():
        _lib.lib().vo_glyph_batch(P(px), P(of), P(iw), P(cod), P(csd), P(cwd), B, H, cell, 0, W, P(out), st)
    t_k = timed(k, 200)
    nbytes = n_in + out.numel() * 4
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 2.0:
        O.glyph_batch(strips, widths, cell, 1)
        n += 1
    t_cpu = (time.perf_counter() - t0) / n
    return {"metric": "glyph batch layout (training input pipeline, SURVEY 8(f) row 2)", "unit": "batches/s",
            "value": round(1 / t_k, 1), "e2e_batches_per_s_incl_host_pack_h2d": round(1 / t_e2e, 1),
            "config": {"batch": B, "cell": cell, "height": H, "out_width": W},
            "roofline": {"bound": "hbm", "achieved": round(nbytes / t_k / 1e9, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(nbytes / t_k / 1e9 / HBM_PEAK_GBS, 4),
                         "bytes_per_launch": nbytes, "avg_launch_us": round(t_k * 1e6, 2)},
            "cpu_baseline": {"value": round(1 / t_cpu, 1), "unit": "batches/s", "cores": 1, "kind": "port",
                             "sample": f"{n} batches, oracle/data.py numpy layout"}}


def features():
    from helpers import configs
    from oracle import mel as O
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    rng = np.random.default_rng(1)
    n_utt, N = 64, 44100
    wavs = [(0.3 * rng.standard_normal(N)).astype(np.float32) for _ in range(n_utt)]
    F = 1 + N // 256
    durs = [np.full(8, (F - 1) // 8) for _ in range(n_utt)]
    fx = FeatureExtractor(configs()[0])
    fx.process(wavs, durs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        fx.process(wavs, durs)
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / reps
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 5.0 and n < n_utt:
        O.char_features(wavs[n], durs[n])
        n += 1
    t_cpu = (time.perf_counter() - t0) / n
    return {"metric": "offline feature extraction (mel + char energy + kurtosis, SURVEY 8(f) row 3)",
            "unit": "utterances/s (2 s @ 22.05 kHz)", "value": round(n_utt / t_gpu, 1),
            "config": {"utterances": n_utt, "samples": N, "frames": F},
            "note": "host-inclusive (numpy in, numpy out per utterance)",
            "cpu_baseline": {"value": round(1 / t_cpu, 1), "unit": "utterances/s", "cores": torch.get_num_threads(),
                             "kind": "port", "sample": f"{n} utterances, oracle/mel.char_features torch-CPU"}}


def _aug_bases():
    """The synthetic corpus of the augment and stats modes -> (rng, configs, bases): 120 utterances of ICASSP-like
    sizes."""
    import copy
    import augment_check as C
    from helpers import DATA, configs
    rng = np.random.default_rng(14)
    pc, mc, tc = copy.deepcopy(configs())
    U, H, cell = 120, 24, 102
    sym = C.symbol_ids()
    chars, labels = list(sym), sorted(json.load(open(os.path.join(DATA, "audiotype.json"))))
    bases = []
    for u in range(U):  # 2 .. 7 characters of 8 .. 40 frames (0.1 .. 0.46 s) and 30 .. 102 pixels; one in three has a run
        n = int(rng.integers(2, 8))
        text = [chars[i] for i in rng.integers(0, len(chars), n)]
        if u % 3 == 0 and n >= 4:
            text[1:4] = [text[1]] * 3
        dur, width = rng.integers(8, 41, n), rng.integers(30, cell + 1, n).astype(np.int32)
        label = labels[u % len(labels)]
        bases.append({"id": f"font_24pt_{label}-a1-{u:03d}", "label": label, "text_str": "".join(text),
                      "audiotype": u % len(labels), "text": np.array([sym[c] for c in text]),
                      "mel": rng.standard_normal((int(dur.sum()), 80)).astype(np.float32),
                      "energy": rng.standard_normal(n), "kurtosis": None, "duration": dur,
                      "image": (rng.integers(0, 256, (H, int(width.sum()))).astype(np.uint8), width),
                      "event_image_feature": None})
    return rng, (pc, mc, tc), bases


def augment(kernels=0):
    import ctypes
    import shutil
    import statistics
    import tempfile
    from pathlib import Path
    from PIL import Image
    import augment_check as C
    from helpers import DATA
    from visual_onoma_to_wave_amd import _lib, ops
    from visual_onoma_to_wave_amd.dataset import Dataset, DeviceCorpus
    from visual_onoma_to_wave_amd.utils.tools import to_device
    rng, (pc, mc, tc), bases = _aug_bases()
    cfg, B, U, H, cell, dev = pc["augmentation"], 48, len(bases), 24, 102, torch.device("cuda")
    sym = C.symbol_ids()
    corpus = DeviceCorpus.from_arrays(bases, cell, pc["visual_text"]["stride"], dev)
    names, plan = corpus.variants(cfg)
    rows = np.sort(rng.choice(len(names), B, replace=False))
    plan_h = plan[rows]
    first = corpus.batch(plan_h)
    T_src, T_mel = first[4], first[7]
    plan_d = torch.from_numpy(plan_h).to(dev)
    static = corpus.batch(plan_d, T_src, T_mel)
    assert all(torch.equal(static[i], first[i]) for i in (1, 2, 3, 5, 6, 8, 10, 11))
    o = dict(zip(ops.AUGMENT_OUT, [static[i] for i in (1, 2, 3, 5, 6, 8, 9, 10, 11)] + [corpus.last_status]))
    P = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    W = static[11].shape[-1]

    fn = _lib.lib().vo_augment_batch
    c_args = (ctypes.byref(corpus.struct), P(plan_d), B, T_src, T_mel, H, cell, corpus.margin, W,
              *[P(o[k]) for k in ops.AUGMENT_OUT], st)

    def launch():  # the launch alone, through the C ABI
        fn(*c_args)
    out_bytes = sum(t.numel() * t.element_size() for t in o.values() if t is not None)
    if kernels:  # for a kernel trace (rocprofv3 --kernel-trace --stats): launches only
        for _ in range(kernels):
            launch()
        torch.cuda.synchronize()
        return {"metric": "augment launches for a kernel trace", "value": kernels, "unit": "launches",
                "bytes_per_launch": out_bytes}

    # the path this replaces: the variants as files, Dataset.__getitem__, collate_fn, to_device
    tmp = Path(tempfile.mkdtemp(prefix="vo_aug_bench_"))
    try:
        for f in ("visual_text.json", "audiotype.json", "symbols.json"):
            shutil.copy(os.path.join(DATA, f), tmp / f)
        lines = []
        for name, (src, pos, m, mm, r) in zip([names[i] for i in rows], plan_h.tolist()):
            u = bases[src]
            v = C.model_row(u, pos, m, mm, r)
            for sub, a in (("mel", v["mel"]), ("energy", v["energy"]), ("duration", v["duration"]),
                           ("image/width", v["image"][1])):
                (tmp / sub / u["label"]).mkdir(parents=True, exist_ok=True)
                np.save(tmp / sub / u["label"] / f"{name}.npy", a)
            (tmp / "image/png" / u["label"]).mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.repeat(v["image"][0][:, :, None], 3, axis=2)).save(tmp / "image/png" / u["label"] / f"{name}.png")
            text = "".join(u["text_str"][c] for c in C.sigma(len(u["text_str"]), pos, m, r))
            lines.append(f"{name}|{u['label']}|24|font|{text}")
        (tmp / "bench.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
        pc["path"]["preprocessed"] = str(tmp)
        tc["optimizer"] = dict(tc["optimizer"], batch_size=B)
        ds = Dataset("bench.txt", pc, tc, mc)

        def host():
            batch = to_device(ds.collate_fn([ds[i] for i in range(B)])[0], dev)
            torch.cuda.synchronize()
            return batch
        want = host()
        assert want[0] == first[0] and all(torch.equal(want[i], first[i]) for i in (1, 2, 3, 5, 6, 8, 10, 11))
        t_host, t_call, t_launch = [], [], []
        for _ in range(5):  # the two paths alternate; windows of 0.1 s and more
            t0 = time.perf_counter()
            for _ in range(3):
                host()
            t_host.append((time.perf_counter() - t0) / 3)
            t_call.append(timed(lambda: corpus.batch(plan_d, T_src, T_mel, out=static), 2000))
            t_launch.append(timed(launch, 5000))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    med = statistics.median
    spread = lambda v: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]  # noqa: E731
    return {"metric": "augmented training batch from a device plan (preprocessor.py:468-622 + collate, DESIGN.md 14)",
            "unit": "batches/s", "value": round(1 / med(t_call), 1),
            "config": {"batch": B, "corpus_utterances": U, "rows_in_corpus_plan": len(names), "T_src": T_src,
                       "T_mel": T_mel, "image_width": W, "n_mels": 80, "windows": 5},
            "device_path": {"corpus.batch_us": round(med(t_call) * 1e6, 2), "corpus.batch_us_min_max": spread(t_call),
                            "launch_us": round(med(t_launch) * 1e6, 2), "launch_us_min_max": spread(t_launch),
                            "note": "back-to-back launches, device events; the 48-row batch stays in the L2 / MALL"},
            "host_path": {"batch_us": round(med(t_host) * 1e6, 1), "batch_us_min_max": spread(t_host),
                          "note": "48 x Dataset.__getitem__ (np.load, PNG decode; files in the page cache), collate_fn, "
                                  "to_device + synchronize, one process"},
            "speedup_corpus.batch_vs_host": round(med(t_host) / med(t_call), 1),
            "roofline": {"bound": "hbm", "achieved": round(out_bytes / med(t_launch) / 1e9, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s of output bytes", "frac": round(out_bytes / med(t_launch) / 1e9 / HBM_PEAK_GBS, 4),
                         "bytes_per_launch": out_bytes}}


def stats():
    """vo_corpus_stats over the whole augmented corpus of the augment mode (its 120 utterances, every row of
    ``corpus.variants``) against the host path it replaces: numpy over the materialised arrays, np.percentile, the
    filter, mean and std."""
    import ctypes
    import statistics
    import corpus_stats_check as S
    from visual_onoma_to_wave_amd import _lib, ops
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    _, (pc, _, _), bases = _aug_bases()
    dev = torch.device("cuda")
    corpus = DeviceCorpus.from_arrays(bases, 102, pc["visual_text"]["stride"], dev)
    names, plan = corpus.variants(pc["augmentation"])
    plan_d = torch.from_numpy(plan).to(dev)
    out, status = ops.corpus_stats(corpus.struct, plan_d, "energy")
    ws = torch.empty(int(_lib.lib().vo_corpus_stats_workspace_size(len(plan))), dtype=torch.uint8, device=dev)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    c_args = (ctypes.byref(corpus.struct), P(plan_d), len(plan), _lib.STATS_ENERGY, P(ws), ws.numel(), P(out),
              P(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = _lib.lib().vo_corpus_stats

    def launch():  # the two launches alone, through the C ABI
        fn(*c_args)
    values = [u["energy"].astype(np.float32) for u in bases]
    arrays = [S.row_array(values[r[0]], r) for r in plan.tolist()]  # the variants materialised once, outside the timing

    def host():
        kept = [S.keep(v) for v in arrays]
        flat = np.concatenate(kept)
        mean = float(flat.mean())
        return len(flat), mean, float(np.sqrt(np.mean((flat - mean) ** 2))), min(float(v.min()) for v in arrays), \
            max(float(v.max()) for v in arrays)
    want, got = host(), out.cpu().numpy()
    assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4] and not bool(status.any())
    assert abs(got[1] - want[1]) <= want[0] * 2.0 ** -52 * (abs(want[1]) + want[2])
    assert abs(got[2] - want[2]) <= want[0] * 2.0 ** -52 * want[2]
    t_host, t_call, t_launch = [], [], []
    for _ in range(5):  # the two paths alternate
        t0 = time.perf_counter()
        for _ in range(3):
            host()
        t_host.append((time.perf_counter() - t0) / 3)
        t_call.append(timed(lambda: ops.corpus_stats(corpus.struct, plan_d, "energy", out=out, status=status,
                                                     workspace=ws), 2000))
        t_launch.append(timed(launch, 5000))
    med = statistics.median
    spread = lambda v: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]  # noqa: E731
    return {"metric": "energy statistics over the augmented corpus from a device plan (preprocessor.py:113-144, "
                      "DESIGN.md 15)", "unit": "calls/s", "value": round(1 / med(t_launch), 1),
            "config": {"corpus_utterances": len(bases), "plan_rows": len(plan), "kept_values": int(want[0]),
                       "characters_in_all_rows": int(sum(len(v) for v in arrays)), "windows": 5},
            "device_path": {"vo_corpus_stats_us": round(med(t_launch) * 1e6, 2),
                            "vo_corpus_stats_us_min_max": spread(t_launch),
                            "ops.corpus_stats_us": round(med(t_call) * 1e6, 2),
                            "ops.corpus_stats_us_min_max": spread(t_call),
                            "note": "back-to-back calls (two launches each), device events"},
            "host_path": {"stats_us": round(med(t_host) * 1e6, 1), "stats_us_min_max": spread(t_host),
                          "note": "numpy over the materialised float64 arrays (built outside the timing): two "
                                  "np.percentile and the filter per array, mean and std of the concatenation, min / max"},
            "speedup_launches_vs_host": round(med(t_host) / med(t_launch), 1)}


def _seg_corpus(dev):
    """The synthetic corpus of the augment mode with int16 waveforms of F * hop samples attached -> (corpus, waves)."""
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    rng, (pc, _, _), bases = _aug_bases()
    hop = 256
    wavs = [rng.integers(-8000, 8001, u["mel"].shape[0] * hop).astype(np.int16) for u in bases]
    corpus = DeviceCorpus.from_arrays(bases, 102, pc["visual_text"]["stride"], dev).attach_waves(wavs, hop)
    return corpus, bases, wavs


def segments():
    """A HiFi-GAN training batch (16 segments of 8192 samples and their 32 mel frames) drawn and cut on the device
    (vo_segment_plan + vo_segment_batch, hifigan.data.SegmentSampler) against the host path it
    replaces: numpy crops of the same rows, torch.from_numpy, .to(device), synchronise."""
    import ctypes
    import statistics
    from visual_onoma_to_wave_amd import _lib
    from visual_onoma_to_wave_amd.hifigan import SegmentSampler
    dev = torch.device("cuda")
    corpus, bases, wavs = _seg_corpus(dev)
    B, seg, hop = 16, 8192, 256
    fps = seg // hop
    s = SegmentSampler(corpus, seg, hop, B, seed=16)
    x, y = s.draw()
    rows = s.plan.cpu().tolist()
    mels = [u["mel"] for u in bases]

    def host():
        hx, hy = np.zeros((B, fps, 80), np.float32), np.zeros((B, seg), np.float32)
        for b, (src, start) in enumerate(rows):
            m = mels[src][start:start + fps]
            a = wavs[src][start * hop:start * hop + seg]
            hx[b, :len(m)] = m
            hy[b, :len(a)] = a.astype(np.float32) / np.float32(32768.0)
        out = torch.from_numpy(hx).to(dev), torch.from_numpy(hy).to(dev)
        torch.cuda.synchronize()
        return out
    hx, hy = host()
    assert torch.equal(hx, x) and torch.equal(hy, y) and not bool(s.status.any())
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.lib()
    plan_args = (ctypes.byref(corpus.struct), P(s.order), s.order.shape[0], P(s.counter), s.seed, B, fps, P(s.plan), st)
    batch_args = (ctypes.byref(corpus.struct), ctypes.byref(corpus.waves), P(s.plan), B, fps, hop, 0.0, P(y), P(x),
                  P(s.frames), P(s.status), st)

    def launch():  # the two launches alone, through the C ABI
        lib.vo_segment_plan(*plan_args)
        lib.vo_segment_batch(*batch_args)
    t_host, t_call, t_launch = [], [], []
    for _ in range(5):  # the two paths alternate
        t0 = time.perf_counter()
        for _ in range(200):
            host()
        t_host.append((time.perf_counter() - t0) / 200)
        t_call.append(timed(s.draw, 2000))
        t_launch.append(timed(launch, 5000))
    med = statistics.median
    spread = lambda v: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]  # noqa: E731
    out_bytes = x.numel() * 4 + y.numel() * 4
    assert med(t_call) <= med(t_host), (med(t_call), med(t_host))  # the device path is not slower than the host's
    return {"metric": "HiFi-GAN training batch drawn and cut on the device (DESIGN.md 16)", "unit": "batches/s",
            "value": round(1 / med(t_call), 1),
            "config": {"batch": B, "segment_size": seg, "hop": hop, "n_mels": 80, "corpus_utterances": len(bases),
                       "waveforms": "int16, F * hop samples", "output_bytes": out_bytes, "windows": 5},
            "device_path": {"sampler.draw_us": round(med(t_call) * 1e6, 2), "sampler.draw_us_min_max": spread(t_call),
                            "launches_us": round(med(t_launch) * 1e6, 2), "launches_us_min_max": spread(t_launch),
                            "note": "back-to-back calls (two launches each: the draw, the cut), device events; "
                                    f"{out_bytes / 1e6:.2f} MB of output: launch latency bounds it, not bandwidth, so no "
                                    "roofline fraction is quoted"},
            "host_path": {"batch_us": round(med(t_host) * 1e6, 1), "batch_us_min_max": spread(t_host),
                          "note": "numpy crops of the same 16 rows from arrays in memory, torch.from_numpy, .to(device), "
                                  "synchronize, one process"},
            "host_over_device": round(med(t_host) / med(t_call), 2)}


def segments_c5():
    """The C5 training step at the benchmark's shape (batch 16, segment 8192, bf16 compute) as one graph replay with
    its batch drawn inside (``step_graphed(sampler=...)``) against the replay over static tensors plus their two
    copies (``step_graphed(x, y)``): five windows each, the order rotated."""
    import statistics
    from helpers import hifigan_arrays, hifigan_h
    from weights import load_into
    from visual_onoma_to_wave_amd import hifigan
    dev = torch.device("cuda")
    corpus, _, _ = _seg_corpus(dev)
    h = hifigan.AttrDict(hifigan_h())
    B, seg, hop, steps = 16, h.segment_size, h.hop_size, 20
    runs = {}
    for kind in ("static", "sampler"):
        g = hifigan.Generator(h)
        load_into(g, hifigan_arrays())
        torch.manual_seed(1234)
        tr = hifigan.HifiGanTrainer(g.to(dev), h, device=dev, graphed=True).set_compute_dtype(torch.bfloat16)
        s = hifigan.SegmentSampler(corpus, seg, hop, B, seed=5)
        if kind == "sampler":
            runs[kind] = lambda tr=tr, s=s: tr.step_graphed(sampler=s)
        else:
            x, y = (t.clone() for t in s.draw())
            runs[kind] = lambda tr=tr, x=x, y=y: tr.step_graphed(x, y)
        runs[kind]()  # warm-up steps and the capture
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    order = list(runs)
    for i in range(5):
        for k in order[i % 2:] + order[:i % 2]:
            ms[k].append(timed(runs[k], steps) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"metric": "C5 step: graph replay with the batch drawn inside against static tensors", "unit": "ms/step",
            "value": round(med["sampler"], 3),
            "config": {"batch": B, "segment": seg, "dtype": "bf16", "steps_per_window": steps, "windows": 5,
                       "order": "rotated from window to window"},
            "ms_per_step": {k: [round(t, 3) for t in v] for k, v in ms.items()},
            "median": {k: round(v, 3) for k, v in med.items()},
            "sampler_minus_static_us": round((med["sampler"] - med["static"]) * 1e3, 1),
            "note": "the sampler's replay holds two more launches (the draw, the cut) and no copies of x and y into "
                    "the static buffers; the static path's two copies are outside its graph"}


def resample():
    """vo_resample at the corpus ingestion shape: B = 64 rows of 2 s at 48000 -> 22050, int16
    in, fp32 out.  Device events over back-to-back launches, five windows, at least 0.5 s of work in all."""
    import statistics
    from visual_onoma_to_wave_amd import ops
    dev = torch.device("cuda")
    B, N, sr_in, sr_out = 64, 96000, 48000, 22050
    O, M, W = ops.resample_geometry(sr_in, sr_out)
    T = 2 * W + 1
    rng = np.random.default_rng(17)
    host = torch.from_numpy(rng.integers(-16384, 16385, (B, N)).astype(np.int16))
    pinned = host.pin_memory()
    x = host.to(dev)
    L = ops.resample_len(N, O, M)
    out = torch.empty((B, L), dtype=torch.float32, device=dev)
    run = lambda: ops.resample(x, sr_in, sr_out, out=out)  # noqa: E731
    run()
    torch.cuda.synchronize()
    t1 = timed(run, 20)
    n = max(20, int(0.12 / t1) + 1)  # 0.12 s a window: 0.6 s of work in all
    t_call = [timed(run, n) for _ in range(5)]
    stage = torch.empty_like(x)

    def upload():
        stage.copy_(pinned, non_blocking=True)
    t_up = [timed(upload, 50) for _ in range(5)]
    med = statistics.median
    t = med(t_call)
    flops = 2.0 * T * B * L
    table_bytes = M * T * 4
    moved = B * N * 2 + B * L * 4 + table_bytes
    tf = flops / t / 1e12
    return {"metric": "sample-rate conversion 48000 -> 22050 on the device (DESIGN.md 17)", "unit": "us/call",
            "value": round(t * 1e6, 1),
            "config": {"rows": B, "samples_in": N, "samples_out": L, "taps": T, "input": "int16", "output": "fp32",
                       "calls_per_window": n, "windows": 5},
            "call_us_min_max": [round(min(t_call) * 1e6, 1), round(max(t_call) * 1e6, 1)],
            "fp32": {"tflops": round(tf, 2), "vector_peak_tflops": FP32_VECTOR_PEAK_TFLOPS,
                     "fraction_of_peak": round(tf / FP32_VECTOR_PEAK_TFLOPS, 4),
                     "bound_us": round(flops / (FP32_VECTOR_PEAK_TFLOPS * 1e12) * 1e6, 1)},
            "bytes": {"algorithmic": moved, "bound_us": round(moved / (HBM_PEAK_GBS * 1e9) * 1e6, 2),
                      "note": "int16 in + fp32 out + the table once, at the HBM peak"},
            "bounded_by": "fp32" if flops / (FP32_VECTOR_PEAK_TFLOPS * 1e12) > moved / (HBM_PEAK_GBS * 1e9)
            else "bytes",
            "seconds_of_audio_per_second": round(B * N / sr_in / t, 1),
            "upload": {"pinned_h2d_us": round(med(t_up) * 1e6, 1),
                       "us_min_max": [round(min(t_up) * 1e6, 1), round(max(t_up) * 1e6, 1)],
                       "note": "the same (64, 96000) int16 batch from pinned host memory, for scale"}}


if __name__ == "__main__":
    args = sys.argv[1:]
    out = args.pop(args.index("--out") + 1) if "--out" in args else None
    kernels = int(args.pop(args.index("--kernels") + 1)) if "--kernels" in args else 0
    args = [a for a in args if a not in ("--out", "--kernels")]
    which = {"glyph": glyph, "features": features, "augment": (lambda: augment(kernels)) if kernels else augment,
             "stats": stats, "segments": segments, "resample": resample, "segments-c5": segments_c5}
    lines = [json.dumps(which[k]()) for k in (args or [k for k in which if k != "segments-c5"])]
    print("\n".join(lines))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
