"""Shared by the ragged mel front-end tests (``vo_stft_mel_lens``): the case table and a float64 reference per row.

The reference restates the kernel's definition on ``x[:n]`` alone -- clip, ``np.pad(mode="reflect")``, window,
``np.fft.rfft``, sqrt(re^2 + im^2 + eps), filterbank product, log floor, frame energy and the two power statistics --
in float64.  ``tests/test_mel_ragged_cpu.py`` pins it to ``oracle.mel`` before the kernel is judged by it."""

import functools

import numpy as np
import torch

from oracle import mel as M
from test_mel import _wav

LOG_FLOOR = 1e-5

# name -> framing, capacity N, the batch's lengths and the frame counts they must give (ISSUE table):
#   centred: the shortest row that can reflect, one sample under a hop multiple, a hop multiple, the full row,
#            n = pad (cannot reflect), empty;  hifigan: the same edges at pad (n_fft - hop) / 2;  small: n_fft 64.
CASES = {
    "centred": dict(n_fft=1024, hop=256, pad=512, mag_eps=0.0, clip=True, N=2048, n_mels=80, fb="htk", seed=11,
                    lens=[513, 767, 768, 2048, 512, 0], frames=[3, 3, 4, 9, 0, 0]),
    "hifigan": dict(n_fft=1024, hop=256, pad=384, mag_eps=1e-9, clip=False, N=2048, n_mels=80, fb="slaney", seed=12,
                    lens=[385, 511, 512, 2048, 384], frames=[1, 1, 2, 8, 0]),
    "small": dict(n_fft=64, hop=16, pad=32, mag_eps=0.0, clip=True, N=300, n_mels=10, fb="htk", seed=13,
                  lens=[33, 47, 48, 300, 32], frames=[3, 3, 4, 19, 0]),
}


def closed_form_frames(n, n_fft, hop, pad):
    return 1 + (n + 2 * pad - n_fft) // hop if (n > pad and n + 2 * pad >= n_fft) else 0


def capacity(c):
    return closed_form_frames(c["N"], c["n_fft"], c["hop"], c["pad"])


@functools.lru_cache(maxsize=None)
def filterbank(name):
    """(n_fft / 2 + 1, n_mels) float32, as the kernel takes it."""
    c = CASES[name]
    if c["fb"] == "htk":
        return M.melscale_fbanks(c["n_fft"] // 2 + 1, 0.0, 8000.0, c["n_mels"], 22050).float().contiguous()
    return torch.from_numpy(M.librosa_mel(22050, c["n_fft"], c["n_mels"], 0.0, 8000.0)).t().contiguous()


def window(name):
    return torch.hann_window(CASES[name]["n_fft"], periodic=True)


@functools.lru_cache(maxsize=None)
def signals(name):
    """(B, N) float32 from test_mel.py's recipe (sines plus noise, slight clipping); read-only."""
    c = CASES[name]
    w = _wav(len(c["lens"]), c["N"], seed=c["seed"])
    w.setflags(write=False)
    return w


def poisoned(name):
    """The batch the kernel gets: every sample past a row's length is NaN."""
    c = CASES[name]
    w = signals(name).copy()
    for b, n in enumerate(c["lens"]):
        w[b, n:] = np.nan
    return w


def reference_row(x, n, c, win, fb):
    """float64 (mel (n_mels, F_b), energy (F_b,), fstats (F_b, 2)) of the n-sample signal x[:n]."""
    n_fft, hop, pad = c["n_fft"], c["hop"], c["pad"]
    Fb = closed_form_frames(n, n_fft, hop, pad)
    if Fb == 0:
        return np.zeros((fb.shape[1], 0)), np.zeros(0), np.zeros((0, 2))
    x = np.asarray(x[:n], np.float64)
    if c["clip"]:
        x = np.clip(x, -1.0, 1.0)
    xp = np.pad(x, (pad, pad), mode="reflect")
    fr = np.stack([xp[f * hop: f * hop + n_fft] for f in range(Fb)]) * np.asarray(win, np.float64)[None]
    X = np.fft.rfft(fr, axis=1)
    mag = np.sqrt(X.real ** 2 + X.imag ** 2 + c["mag_eps"])              # (F_b, bins)
    mel = np.log(np.maximum(mag @ np.asarray(fb, np.float64), LOG_FLOOR)).T
    p = mag * mag
    return mel, np.sqrt(p.sum(1)), np.stack([p.sum(1), np.log(p + 1e-8).sum(1)], axis=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per row of the case: reference_row on the clean signal; computed once, shared by the tests."""
    c = CASES[name]
    w, win, fb = signals(name), window(name).numpy(), filterbank(name).numpy()
    return tuple(reference_row(w[b], n, c, win, fb) for b, n in enumerate(c["lens"]))


def fstats_rel_err(got, ref):
    """max |got - ref| / |ref| over both statistics of every frame."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref))) if ref.size else 0.0
