"""Offline acoustic feature extraction on the GPU: the producer of the
``mel/*.npy`` (T, 80), ``energy/*.npy`` and ``kurtosis/*.npy`` character-level features and
their corpus z-normalisation that the training Dataset reads.

Reference: scripts/preprocessor/preprocessor.py -- ``Preprocessor._get_spec`` (:323-337,
torchaudio Spectrogram(power=1, center=True) + MelScale(slaney) + log clamp 1e-5, energy = L2
norm of |X| over frequency), the frame -> character energy averaging of ``_process``
(:395-403), ``_get_kurtosis`` (:339-357) and the StandardScaler + ``_normalize`` pass of
``build_from_path`` (:113-129, :624-645), and the first two steps of ``_process``: the resampling of
``librosa.load(path, sr=22050)`` (:385) and the trim ``wav[int(sr * start):]`` (:391), as one ``vo_resample`` launch
per source rate (``process(..., sr=, start=)``; DESIGN.md section 17 states the rule -- parity with librosa's
resampler is unpinned).  Corpus walking, reading the files (``audio.read_wav``), TextGrid alignment and glyph
rendering stay host-side and are out of scope.

GPU work per call (per chunk under ``max_batch_samples``): the utterances, whatever their lengths, are padded
into one (B, N_max) batch; one ``vo_stft_mel_lens`` launch (framing per signal length, FFT, |X|, mel
channels-last, log, frame energy and the power statistics the kurtosis needs), one ``vo_char_features``
launch (per-character reductions over the duration spans) and one device-to-host copy per output kind.  Utterances
at another rate than the config's are resampled, one launch per rate, straight into that (B, N_max) batch, whose
lengths the mel launch then reads from the device: no host round trip in between.
"""

import numpy as np
import torch

from .. import ops
from ..audio import melscale_fbanks, pad_waves, padded_window


class FeatureExtractor:
    def __init__(self, config, device="cuda", max_batch_samples=None):
        """``max_batch_samples``: split a ``process`` call into several launches when B * N_max of the padded
        batch would exceed it, so that one long clip does not pad a thousand short ones (None: one launch)."""
        a = config["audio"]
        st, mel = a["stft"], a["mel"]
        self.n_fft, self.hop, self.win = st["filter_length"], st["hop_length"], st["win_length"]
        self.n_mels = mel["n_mel_channels"]
        self.max_batch_samples = max_batch_samples
        self.sr = int(a["sampling_rate"])
        self.device = torch.device(device)
        self.fb = melscale_fbanks(self.n_fft // 2 + 1, mel["mel_fmin"], mel["mel_fmax"], self.n_mels,
                                  a["sampling_rate"]).float().contiguous().to(self.device)
        self.window = padded_window(self.win, self.n_fft).to(self.device)

    def get_spec(self, audio):
        """Preprocessor._get_spec: 1-D waveform -> (log-mel (80, F), energy (F,)) numpy."""
        w = torch.as_tensor(np.asarray(audio, np.float32), device=self.device)[None].contiguous()
        mel, energy, _ = ops.spec_features(w, self.window, self.fb, self.n_fft, self.hop)
        return mel[0].cpu().numpy(), energy[0].cpu().numpy()

    def _chunks(self, lens):
        """Consecutive index runs whose padded size B * N_max stays within max_batch_samples (a single utterance
        longer than that is a run of its own)."""
        if self.max_batch_samples is None:
            return [list(range(len(lens)))]
        runs, cur, n_max = [], [], 0
        for i, n in enumerate(lens):
            if cur and (len(cur) + 1) * max(n_max, n) > self.max_batch_samples:
                runs.append(cur)
                cur, n_max = [], 0
            cur.append(i)
            n_max = max(n_max, n)
        if cur:
            runs.append(cur)
        return runs

    def _batch(self, wavs, rates, skips, out_lens):
        """The chunk's padded batch on the device: (wav (B, N_max) fp32, lens (B,) int32, order).  Row k holds
        utterance order[k]: the utterances already at the config's rate first (trimmed and padded on the host, one
        copy), then one group per source rate, each resampled in one launch into its rows of the buffer."""
        same = [i for i, r in enumerate(rates) if r == self.sr]
        if len(same) == len(wavs):
            wav, wl = pad_waves([w[k:] for w, k in zip(wavs, skips)])
            return wav.to(self.device), wl.to(self.device), same
        B, N_max = len(wavs), max(max(out_lens), 1)
        buf = torch.zeros((B, N_max), dtype=torch.float32, device=self.device)
        order, lens = list(same), []
        if same:
            wav, wl = pad_waves([wavs[i][skips[i]:] for i in same])
            buf[:len(same), :wav.shape[1]] = wav.to(self.device)
            lens.append(wl.to(self.device))
        for rate in sorted(set(rates) - {self.sr}):
            idx = [i for i, r in enumerate(rates) if r == rate]
            wav, wl = pad_waves([wavs[i] for i in idx])
            a = len(order)
            _, n = ops.resample(wav.to(self.device), rate, self.sr, lens=wl.tolist(), skip=[skips[i] for i in idx],
                                out=buf[a:a + len(idx)])
            lens.append(n)
            order += idx
        return buf, torch.cat(lens), order

    def process(self, wavs, durations, sr=None, start=None, return_wavs=False):
        """Batch of utterances (1-D float arrays, trimmed as in _process) and their per-character
        durations (frames) -> list of dicts {mel (sum(d), 80), energy (n_chars,), kurtosis (n_chars,)}
        exactly as _process saves them (mel transposed, truncated to sum(duration)).  Each utterance is
        framed as a signal of its own length (reflect padding is per signal): its results do not depend on
        what it is batched with.

        ``sr``: the rate the arrays are at, an int or one per utterance (None: the config's ``sampling_rate``).
        Utterances at another rate are resampled to it on the device (``ops.resample``), which is the reference's
        ``librosa.load(path, sr=sampling_rate)``; a ratio the library does not run is a ValueError.  ``start``
        (seconds, one per utterance): the first ``int(sampling_rate * start)`` samples at the config's rate are
        dropped, the reference's ``wav[int(sr * start):]``.  The durations are checked against the resampled, trimmed
        length, on the host and before any launch.  ``return_wavs``: each dict also holds ``wav``, the fp32 signal
        the features were taken from.  int16 arrays (``audio.read_wav``) are PCM: s / 32768."""
        if len(durations) != len(wavs):
            raise ValueError(f"process: {len(wavs)} utterances, {len(durations)} duration lists")
        n_utt = len(wavs)
        wavs = [np.asarray(w) for w in wavs]
        wavs = [(w.astype(np.float32) / np.float32(32768.0)) if w.dtype == np.int16 else w for w in wavs]
        rates = [self.sr] * n_utt if sr is None else [int(sr)] * n_utt if np.ndim(sr) == 0 else [int(r) for r in sr]
        starts = [0.0] * n_utt if start is None else [float(v) for v in start]
        if len(rates) != n_utt or len(starts) != n_utt:
            raise ValueError(f"process: {n_utt} utterances, {len(rates)} rates, {len(starts)} start times")
        if any(not (v >= 0.0 and v < float("inf")) for v in starts):
            raise ValueError(f"process: start times must be finite and >= 0, got {starts}")
        skips = [int(self.sr * v) for v in starts]
        geo = {r: ops.resample_geometry(r, self.sr) for r in set(rates) - {self.sr}}  # refusals, before any launch
        lens = [max((len(w) if r == self.sr else ops.resample_len(len(w), *geo[r][:2])) - k, 0)
                for w, r, k in zip(wavs, rates, skips)]
        T = [int(np.sum(d)) for d in durations]
        for i, (n, t) in enumerate(zip(lens, T)):  # host check, before any launch
            F_i = ops.stft_mel_frames(n, self.n_fft, self.hop, self.n_fft // 2)
            if t > F_i:
                raise ValueError(f"process: utterance {i}: durations sum to {t} frames, its {n} samples give {F_i}")
        res = [None] * n_utt
        for idx in self._chunks(lens):
            wav, wl, order = self._batch([wavs[i] for i in idx], [rates[i] for i in idx], [skips[i] for i in idx],
                                         [lens[i] for i in idx])
            idx = [idx[k] for k in order]
            mel, energy, fstats, _ = ops.stft_mel_lens(wav, self.window, self.fb, wl, self.n_fft, self.hop, clip=True,
                                                       channels_last=True, want_fstats=True)
            e_c, k_c, off = ops.char_features(energy, fstats, [durations[i] for i in idx], self.n_fft // 2 + 1,
                                              flat=True)
            e_h, k_h = e_c.cpu().numpy(), k_c.cpu().numpy()  # one copy per output kind
            mel_h = mel.cpu().numpy()
            wav_h = wav.cpu().numpy() if return_wavs else None
            for j, i in enumerate(idx):
                res[i] = dict(mel=mel_h[j, :T[i]].copy(), energy=e_h[off[j]:off[j + 1]].copy(),
                              kurtosis=k_h[off[j]:off[j + 1]].astype(np.float64))
                if return_wavs:
                    res[i]["wav"] = wav_h[j, :lens[i]].copy()
        return res


def iqr_inliers(values):
    """``Preprocessor._remove_outlier`` (preprocessor.py:647-660): the values strictly inside the fences 1.5
    interquartile ranges below the 25th and above the 75th percentile (``np.percentile``'s default method).  An
    array whose quartiles coincide keeps nothing."""
    values = np.array(values)
    p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
    lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
    return values[np.logical_and(values > lower, values < upper)]


def normalize_features(arrays, remove_outlier=False):
    """StandardScaler.partial_fit over every value + _normalize: returns (normalised arrays,
    mean, std, min, max) with the population std (ddof 0) StandardScaler uses.
    ``remove_outlier``: mean and std are taken over what ``iqr_inliers`` keeps of each array (an array that
    keeps nothing is skipped), as ``build_from_path`` does (:117-125); every value is still normalised, and min and
    max are over all of them.  The device form over an augmented corpus: ``DeviceCorpus.stats`` (DESIGN.md section
    15)."""
    fit = arrays
    if remove_outlier:
        fit = [iqr_inliers(np.asarray(a, np.float64).reshape(-1)) for a in arrays]
        if not sum(len(a) for a in fit):
            raise ValueError("normalize_features: the outlier rule keeps no value of any array")
    flat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in fit])
    mean = float(flat.mean())
    std = float(np.sqrt(np.mean((flat - mean) ** 2)))
    if std == 0.0:
        std = 1.0  # StandardScaler's handling of a zero variance
    normed = [(np.asarray(a) - mean) / std for a in arrays]
    mn = min(float(np.min(v)) for v in normed)
    mx = max(float(np.max(v)) for v in normed)
    return normed, mean, std, mn, mx
