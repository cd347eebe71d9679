"""Golden vector for win_length < filter_length, from the reference's own STFT.

Runs only where the reference is mounted (see make_goldens.py, whose ``import_reference`` and ``save`` this reuses).
The reference's ``STFT(filter_length, hop_length, win_length)`` (scripts/audio/stft.py:18-50) windows its DFT basis
with ``pad_center(get_window("hann", win_length, fftbins=True), filter_length)`` and ``STFT.transform`` (:52-81)
reflect-pads by filter_length / 2 and convolves with it.  This runs that code on CPU for filter_length 1024,
win_length 800, hop 256 on B = 2 signals of N = 4001 samples in [-1, 1] and writes, as data only,

    stft_ref_win800.npz     wav (2, 4001), window (1024,) -- the padded window the reference built --, magnitude
                            (2, 513, 16)

As in ``make_goldens.stft_goldens``: ``Tensor.cuda`` is the identity for the call (stft.py:68-69 hard-codes
``.cuda()``) and, librosa being absent, ``pad_center`` is its published definition (zeros split (size - n) // 2 left,
the rest right).

    python tests/golden/make_goldens_win.py
"""

import numpy as np

import make_goldens as MG

FILTER, WIN, HOP, B, N = 1024, 800, 256, 2, 4001


def main():
    MG.import_reference()
    import utils.tools  # noqa: F401  (imports the reference's audio package as its main() does)
    import torch
    import audio.stft as ref_stft
    ref_stft.pad_center = lambda w, size: np.pad(w, ((size - len(w)) // 2, size - len(w) - (size - len(w)) // 2))
    stft = ref_stft.STFT(FILTER, HOP, WIN)
    window = ref_stft.pad_center(ref_stft.get_window("hann", WIN, fftbins=True), FILTER)
    rng = np.random.default_rng(800)
    t = np.arange(N) / 22050.0
    f0 = rng.uniform(80, 2000, size=(B, 1))
    wav = 0.5 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 3.1 * f0 * t) + 0.1 * rng.standard_normal((B, N))
    wav = np.clip(wav, -1, 1).astype(np.float32)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            mag, _ = stft.transform(torch.from_numpy(wav))
    finally:
        torch.Tensor.cuda = real_cuda
    assert mag.shape == (B, FILTER // 2 + 1, 1 + N // HOP), mag.shape
    MG.save("stft_ref_win800", wav=wav, window=np.asarray(window, np.float32), magnitude=MG.t2n(mag))


if __name__ == "__main__":
    main()
