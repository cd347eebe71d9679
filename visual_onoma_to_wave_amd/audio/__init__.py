"""Mel / STFT front-end on the HIP ``vo_stft_mel`` kernel.

get_spec / MelSpectrogram  <- scripts/preprocessor/preprocessor.py:22-36,323-337 (torchaudio
                              Spectrogram(power=1, center=True) + MelScale(norm="slaney",
                              mel_scale="htk") + log(clamp_min(., 1e-5)); energy = ||X||_2)
TacotronSTFT               <- scripts/audio/stft.py:130-178 (librosa slaney-scale mel basis,
                              dynamic_range_compression = log(clamp(x, 1e-5)))
The filterbanks are built once on the host (float64 -> float32, the published torchaudio /
librosa formulas); the per-frame work -- framing, window, FFT, |X|, mel projection, log,
energy -- is one kernel launch.
"""

import numpy as np
import torch

from .. import ops


def _hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """torchaudio.functional.melscale_fbanks(norm="slaney", mel_scale="htk") -> (n_freqs, n_mels)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(float(_hz_to_mel_htk(f_min)), float(_hz_to_mel_htk(f_max)), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    fb = torch.clamp(torch.minimum((-slopes[:, :-2]) / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)
    return fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]


def _hz_to_mel_slaney(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    mel = f / f_sp
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, mel)


def _mel_to_hz_slaney(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def librosa_mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """librosa.filters.mel(htk=False, norm="slaney") -> (n_mels, 1 + n_fft // 2) float32."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz_slaney(np.linspace(_hz_to_mel_slaney(fmin), _hz_to_mel_slaney(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2), np.float64)
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def padded_window(win_length, n_fft):
    """The periodic Hann window of ``win_length`` samples centred in ``n_fft``: (n_fft - win_length) // 2 zeros on
    the left, the rest on the right -- what torch.stft / torchaudio Spectrogram do with win_length < n_fft, and the
    reference's pad_center(get_window("hann", win_length, fftbins=True), filter_length) (scripts/audio/stft.py:41-43)."""
    if not 0 < win_length <= n_fft:
        raise ValueError(f"win_length ({win_length}) must lie in [1, n_fft = {n_fft}]")
    w = torch.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = torch.hann_window(win_length, periodic=True)
    return w


def pad_waves(wavs):
    """List of 1-D waveforms -> (wav (B, N_max) fp32 host tensor, zero-filled; lens int32 (B,)): the ragged batch
    ``MelSpectrogram(wav, lengths)`` / ``ops.stft_mel_lens`` take."""
    arrs = [np.asarray(w, np.float32).reshape(-1) for w in wavs]
    lens = np.array([len(a) for a in arrs], np.int32)
    out = np.zeros((len(arrs), int(lens.max()) if len(arrs) else 0), np.float32)
    for i, a in enumerate(arrs):
        out[i, :len(a)] = a
    return torch.from_numpy(out), torch.from_numpy(lens)


def read_wav(path):
    """A PCM ``.wav`` file -> (samples, rate), with the standard library's ``wave``.  16-bit mono comes back as the
    file holds it, int16 (N,); several channels are averaged in float32 on the host (librosa's ``mono=True``: the
    samples / 32768, then the mean), a float32 (N,) array.  Any other sample width is a ValueError naming the file."""
    import wave
    with wave.open(str(path), "rb") as f:
        width, channels, rate, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
        if width != 2:
            raise ValueError(f"read_wav: {path}: {8 * width}-bit samples (16-bit PCM only)")
        data = np.frombuffer(f.readframes(n), dtype="<i2").astype(np.int16, copy=False)
    if channels == 1:
        return data.copy(), rate
    frames = data[:data.size // channels * channels].reshape(-1, channels)
    return (frames.astype(np.float32) / np.float32(32768.0)).mean(axis=1, dtype=np.float32), rate


def resample_length(n, sr_in, sr_out):
    """The samples ``n`` samples at ``sr_in`` become at ``sr_out``: ceil(n M / O) of the reduced rates (n itself
    for equal rates)."""
    if int(sr_in) == int(sr_out):
        return int(n)
    O, M, _ = ops.resample_geometry(sr_in, sr_out)
    return ops.resample_len(n, O, M)


class Resample:
    """Sample-rate conversion on HIP (``ops.resample``: a Kaiser-windowed sinc of 64 zero crossings, the parameters
    torchaudio documents for ``sinc_interp_kaiser`` as resampy's ``kaiser_best``).  The rates are checked here: a
    ratio the library does not run is a ValueError at construction."""

    def __init__(self, sr_in, sr_out):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.geometry = None if self.sr_in == self.sr_out else ops.resample_geometry(self.sr_in, self.sr_out)

    def __call__(self, wav, lengths=None, skip=None):
        """wav (N,) or (B, N), fp32 or int16 (read as s / 32768), on the GPU -> (wav, lengths) at ``sr_out``: fp32
        (N',) / (B, N') with N' = resample_length(N) and the device int32 sample counts of the rows, zeros past
        them.  ``lengths`` / ``skip`` (output samples dropped from the front): as ``ops.resample`` takes them.
        With equal rates the input comes back untouched, with ``lengths`` as given."""
        if self.geometry is None:
            return wav, lengths
        squeeze = wav.dim() == 1
        y, n = ops.resample(wav.reshape(1, -1) if squeeze else wav, self.sr_in, self.sr_out, lens=lengths, skip=skip)
        return (y[0], n[0]) if squeeze else (y, n)


class MelSpectrogram:
    """Spectrogram(n_fft, win_length, hop, power=1, center=True) -> MelScale -> log, on HIP."""

    def __init__(self, n_fft=1024, hop_length=256, n_mels=80, sample_rate=22050, f_min=0.0, f_max=8000.0,
                 fb=None, log_floor=1e-5, win_length=None):
        self.n_fft, self.hop, self.n_mels, self.log_floor = n_fft, hop_length, n_mels, log_floor
        self.fb = (melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate) if fb is None
                   else torch.as_tensor(fb)).float().contiguous()
        self.window = padded_window(n_fft if win_length is None else win_length, n_fft)
        self._dev = {}

    def _on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.window.to(device), self.fb.to(device).contiguous())
        return self._dev[key]

    def __call__(self, wav, lengths=None, channels_last=False):
        """wav (N,) or (B, N) fp32 on the GPU -> (log-mel (B, n_mels, F), energy (B, F)).  With ``lengths`` (B sample
        counts: int32 / int64 device tensor, never read on the host, or a host sequence) the batch is ragged:
        -> (log-mel, energy, frames); row b holds the frames[b] frames of wav[b, :lengths[b]] alone, bit for bit,
        then zeros (``ops.stft_mel_lens``).  ``channels_last``: log-mel as (B, F, n_mels), the vocoder's input."""
        squeeze = wav.dim() == 1
        w = wav.reshape(1, -1) if squeeze else wav
        window, fb = self._on(w.device)
        if lengths is None and not channels_last:
            logmel, energy = ops.stft_mel(w.float().contiguous(), window, fb, self.n_fft, self.hop, self.n_mels,
                                          self.log_floor)
            return (logmel[0], energy[0]) if squeeze else (logmel, energy)
        logmel, energy, _, frames = ops.stft_mel_lens(w.float().contiguous(), window, fb, lengths, self.n_fft,
                                                      self.hop, clip=True, log_floor=self.log_floor,
                                                      channels_last=channels_last)
        if lengths is None:
            return (logmel[0], energy[0]) if squeeze else (logmel, energy)
        return (logmel[0], energy[0], frames[0]) if squeeze else (logmel, energy, frames)


def get_spec(wav, preprocess_config=None):
    """Preprocessor._get_spec: (log-mel (80, F), energy (F,)) of a 1-D waveform."""
    a = (preprocess_config or {}).get("audio", {})
    st, mel = a.get("stft", {}), a.get("mel", {})
    m = MelSpectrogram(st.get("filter_length", 1024), st.get("hop_length", 256), mel.get("n_mel_channels", 80),
                       a.get("sampling_rate", 22050), mel.get("mel_fmin", 0), mel.get("mel_fmax", 8000),
                       win_length=st.get("win_length"))
    return m(wav)


class TacotronSTFT(torch.nn.Module):
    """TacotronSTFT with the librosa slaney mel basis; mel_spectrogram(y) -> (mel, energy)."""

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin,
                 mel_fmax):
        super().__init__()
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        basis = torch.from_numpy(librosa_mel(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax))
        self.register_buffer("mel_basis", basis)
        self._mel = MelSpectrogram(filter_length, hop_length, n_mel_channels, fb=basis.t().contiguous(),
                                   win_length=win_length)

    def mel_spectrogram(self, y, lengths=None):
        """(mel, energy) of y (B, N) in [-1, 1]; with ``lengths`` (see MelSpectrogram) -> (mel, energy, frames) of
        the ragged batch, without the host-side range check (it would read the device)."""
        if lengths is not None:
            return self._mel(y, lengths)
        if float(y.min()) < -1 or float(y.max()) > 1:
            raise AssertionError("waveform must lie in [-1, 1]")
        return self._mel(y)
