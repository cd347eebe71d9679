"""The numpy model of the vocoder's segment kernels (vo_segment_batch, vo_segment_plan; include/vonoma.h, DESIGN.md
section 16): plain loops over the stated rules, one element at a time, written without looking at
visual_onoma_to_wave_amd/hifigan/data.py.  tests/test_segments_cpu.py holds that module's host functions against this
one, tests/test_gpu_segments.py the kernels."""

import numpy as np

MASK = (1 << 32) - 1
# counter words, key words, output words (the issue's table; the first two are Random123's own known answers)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(ctr, key):
    """Philox4x32-10: ten rounds, the key raised by the Weyl constants between them."""
    ctr, key = list(ctr), list(key)
    for r in range(10):
        if r:
            key = [(key[0] + 0x9E3779B9) & MASK, (key[1] + 0xBB67AE85) & MASK]
        a = 0xD2511F53 * ctr[0]
        b = 0xCD9E8D57 * ctr[2]
        ctr = [((b >> 32) ^ ctr[1] ^ key[0]) & MASK, b & MASK, ((a >> 32) ^ ctr[3] ^ key[1]) & MASK, a & MASK]
    return tuple(ctr)


def model_plan(order, counter, seed, B, fps, n_frames):
    """Rows ``src, start`` for k = counter .. counter + B - 1 -> int32 (B, 2)."""
    rows = []
    for b in range(B):
        k = counter + b
        src = int(order[k % len(order)])
        if src < 0 or src >= len(n_frames):
            rows.append((src, 0))
            continue
        F = n_frames[src]
        span = F - fps + 1 if F > fps else 1
        w = philox((k & MASK, k >> 32, 0, 0), (seed & MASK, seed >> 32))[0]
        rows.append((src, (w * span) >> 32))
    return np.asarray(rows, np.int32).reshape(B, 2)


def model_batch(mels, wavs, plan, fps, hop, mel_pad=0.0, max_wav_value=32768.0):
    """``mels``: one (F, n_mels) float32 array per utterance, ``wavs``: one 1-D int16 or float32 array each ->
    {"y", "x", "frames", "status"} as vo_segment_batch writes them."""
    B, n_mels, U = len(plan), mels[0].shape[1], len(mels)
    y = np.zeros((B, fps * hop), np.float32)
    x = np.full((B, fps, n_mels), np.float32(mel_pad), np.float32)
    frames, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (src, start) in enumerate(np.asarray(plan).tolist()):
        if src < 0 or src >= U or start < 0 or start > max(mels[src].shape[0] - fps, 0):
            status[b] = 1
            continue
        F, N, wav = mels[src].shape[0], len(wavs[src]), wavs[src]
        for i in range(fps * hop):
            j = start * hop + i
            if j < N:
                y[b, i] = wav[j].astype(np.float32) / np.float32(max_wav_value) if wav.dtype == np.int16 else wav[j]
        for f in range(fps):
            if start + f < F:
                x[b, f] = mels[src][start + f]
        frames[b] = min(fps, F - start)
    return {"y": y, "x": x, "frames": frames, "status": status}


def utterances(mels):
    """The dicts ``DeviceCorpus.from_arrays`` packs, for mels alone: one character that lasts the whole utterance, a
    strip of two rows and three columns."""
    return [{"id": f"u{i}", "audiotype": 0, "text": np.array([1]), "mel": m, "energy": None, "kurtosis": None,
             "duration": np.array([m.shape[0]]), "image": (np.full((2, 3), 255, np.uint8), np.array([3], np.int32))}
            for i, m in enumerate(mels)]


def make(Fs, Ns, n_mels, kind, seed):
    """Random mels of ``Fs`` frames and waveforms of ``Ns`` samples.  ``kind`` "int16": PCM that holds -32768 and
    32767 wherever two samples fit; "float32": values well outside [-1, 1]."""
    rng = np.random.default_rng(seed)
    mels = [rng.standard_normal((F, n_mels)).astype(np.float32) for F in Fs]
    wavs = []
    for N in Ns:
        if kind == "int16":
            w = rng.integers(-32768, 32768, N).astype(np.int16)
            if N >= 2:
                w[0], w[-1] = -32768, 32767
        else:
            w = (3.0 * rng.standard_normal(N)).astype(np.float32)
        wavs.append(w)
    return mels, wavs
