"""The mel front end with one length per signal (``vo_stft_mel_lens``): row b of a ragged batch is, bit for bit, what
the dense entry gives on ``wav[b, :n_b]`` alone, followed by exact zeros; no sample past n_b is read (they are NaN
here) and no output element is left unwritten (the outputs are handed in NaN-filled).  Cases, signals and the
float64 reference: ``tests/mel_ragged_check.py`` (pinned to the oracle by ``tests/test_mel_ragged_cpu.py``).

Bars against the float64 reference: log-mel and energy as ``tests/test_mel.py``'s ``_check``.  The two frame
statistics (sum p, sum log(p + 1e-8) over the bins) had no bar in the project: on these signals the dense kernel
``vo_stft_mel_ex`` of the commit before this entry, run per row on an MI355X, is within FSTATS_DENSE_ERR = 9.642e-6
relative of the reference (worst frame of the three cases: sum log 9.642e-6 in "centred", 6.8e-7 "hifigan", 1.03e-6
"small"; sum p 2.0e-7, 1.3e-7, 1.6e-7); the bar is 4 times that, FSTATS_BAR = 3.857e-5."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import mel_ragged_check as R
from oracle import mel as M
from test_mel import _check, _wav

pytestmark = pytest.mark.gpu

FSTATS_DENSE_ERR = 9.642e-6
FSTATS_BAR = 4 * FSTATS_DENSE_ERR


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _operands(name):
    """(window, filterbank) on the device, copied once (not inside a graph capture)."""
    return R.window(name).cuda(), R.filterbank(name).cuda()


def _lens_call(name, wav, lens, channels_last=False, prealloc=True):
    """ops.stft_mel_lens on a case's framing, fstats on, into NaN-filled outputs."""
    from visual_onoma_to_wave_amd import ops
    c = R.CASES[name]
    win, fb = _operands(name)
    B, F, nm = wav.shape[0], R.closed_form_frames(wav.shape[1], c["n_fft"], c["hop"], c["pad"]), c["n_mels"]
    pre = dict(mel=_nan(B, F, nm) if channels_last else _nan(B, nm, F), energy=_nan(B, F),
               fstats=_nan(B, F, 2)) if prealloc else dict(want_fstats=True)
    out = ops.stft_mel_lens(wav, win, fb, lens, c["n_fft"], c["hop"], c["pad"], c["mag_eps"], c["clip"],
                            channels_last=channels_last, **pre)
    if prealloc:
        assert out[0] is pre["mel"] and out[1] is pre["energy"] and out[2] is pre["fstats"]
    return out


def _dense(name, wav):
    """vo_stft_mel_ex itself with every output (ops.stft_mel_ex returns the mel only, ops.spec_features is the
    centred framing only) -> (mel (B, n_mels, F), energy, fstats), NaN-filled before the call."""
    from visual_onoma_to_wave_amd import _lib
    c = R.CASES[name]
    win, fb = _operands(name)
    B, N = wav.shape
    F = R.closed_form_frames(N, c["n_fft"], c["hop"], c["pad"])
    mel, e, fs = _nan(B, c["n_mels"], F), _nan(B, F), _nan(B, F, 2)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.lib().vo_stft_mel_ex(p(wav), B, N, p(win), p(fb), c["n_fft"], c["hop"], c["n_mels"], c["pad"],
                                         float(c["mag_eps"]), int(c["clip"]), R.LOG_FLOOR, p(mel), p(e), p(fs),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vo_stft_mel_ex")
    return mel, e, fs


@functools.lru_cache(maxsize=None)
def _ragged(name):
    """The case's ragged call (int32 device lengths, NaN past every row's end), computed once: host tensors."""
    import visual_onoma_to_wave_amd  # noqa: F401  (before the first GPU call)
    wav = torch.from_numpy(R.poisoned(name)).cuda()
    lens = torch.tensor(R.CASES[name]["lens"], dtype=torch.int32, device="cuda")
    return tuple(t.cpu() for t in _lens_call(name, wav, lens))


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("name", list(R.CASES))
def test_edge_lengths(name):
    from visual_onoma_to_wave_amd import ops
    c = R.CASES[name]
    mel, energy, fstats, frames = _ragged(name)
    F = R.capacity(c)
    assert mel.shape == (len(c["lens"]), c["n_mels"], F) and frames.dtype == torch.int32
    assert frames.tolist() == c["frames"]
    for t in (mel, energy, fstats):
        assert not torch.isnan(t).any()
    wav = torch.from_numpy(R.signals(name).copy()).cuda()
    win, fb = _operands(name)
    worst = 0.0
    for b, (n, Fb) in enumerate(zip(c["lens"], c["frames"])):
        # past the row's end: exact zeros (positive: the bytes of 0.0f)
        for t in (mel[b, :, Fb:], energy[b, Fb:], fstats[b, Fb:]):
            assert _same_bits(t, torch.zeros_like(t)), (b, n)
        if Fb == 0:
            continue
        # the row's own frames: the dense entry on wav[b, :n] alone, bit for bit
        row = wav[b:b + 1, :n].contiguous()
        d_mel, d_e, d_fs = _dense(name, row)
        assert d_mel.shape == (1, c["n_mels"], Fb)
        assert _same_bits(mel[b:b + 1, :, :Fb], d_mel), (b, n)
        assert _same_bits(energy[b:b + 1, :Fb], d_e), (b, n)
        assert _same_bits(fstats[b:b + 1, :Fb], d_fs), (b, n)
        assert _same_bits(d_mel, ops.stft_mel_ex(row, win, fb, c["n_fft"], c["hop"], c["n_mels"], c["pad"],
                                                 c["mag_eps"], c["clip"]))
        if name == "centred":
            s_mel, s_e, s_fs = ops.spec_features(row, win, fb, c["n_fft"], c["hop"])
            assert _same_bits(d_mel, s_mel) and _same_bits(d_e, s_e) and _same_bits(d_fs, s_fs)
        # and the float64 reference, under test_mel.py's bars
        r_mel, r_e, r_fs = R.reference(name)[b]
        _check(mel[b, :, :Fb], energy[b, :Fb], torch.from_numpy(r_mel), torch.from_numpy(r_e))
        err = R.fstats_rel_err(fstats[b, :Fb].numpy(), r_fs)
        print(f"{name} row {b} (n = {n}): fstats rel err {err:.3e}")
        worst = max(worst, err)
    print(f"{name}: worst fstats rel err {worst:.3e}, bar {FSTATS_BAR:.3e}")
    assert worst < FSTATS_BAR


@pytest.mark.parametrize("name", list(R.CASES))
def test_channels_last_is_the_transpose(name):
    mel = _ragged(name)[0]
    wav = torch.from_numpy(R.poisoned(name)).cuda()
    lens = torch.tensor(R.CASES[name]["lens"], dtype=torch.int32, device="cuda")
    cl, energy, fstats, frames = _lens_call(name, wav, lens, channels_last=True)
    assert cl.shape == (mel.shape[0], mel.shape[2], mel.shape[1])
    assert _same_bits(cl.transpose(1, 2), mel)
    assert _same_bits(energy, _ragged(name)[1]) and _same_bits(fstats, _ragged(name)[2])
    assert frames.tolist() == R.CASES[name]["frames"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_lens_none_is_the_dense_entry(name):
    from visual_onoma_to_wave_amd import ops
    c = R.CASES[name]
    wav = torch.from_numpy(R.signals(name).copy()).cuda()
    win, fb = _operands(name)
    mel, energy, fstats, frames = _lens_call(name, wav, None)
    d_mel, d_e, d_fs = _dense(name, wav)
    assert _same_bits(mel, d_mel) and _same_bits(energy, d_e) and _same_bits(fstats, d_fs)
    assert _same_bits(mel, ops.stft_mel_ex(wav, win, fb, c["n_fft"], c["hop"], c["n_mels"], c["pad"], c["mag_eps"],
                                           c["clip"]))
    assert frames.tolist() == [R.capacity(c)] * len(c["lens"])
    # outputs not handed in: allocated by the call, energy on request only
    m2, e2, f2, _ = ops.stft_mel_lens(wav, win, fb, None, c["n_fft"], c["hop"], c["pad"], c["mag_eps"], c["clip"],
                                      want_energy=False)
    assert _same_bits(m2, d_mel) and e2 is None and f2 is None


def test_int64_and_host_lengths():
    name = "centred"
    c = R.CASES[name]
    wav = torch.from_numpy(R.poisoned(name)).cuda()
    want = _ragged(name)
    for lens in (torch.tensor(c["lens"], dtype=torch.int64, device="cuda"), list(c["lens"]),
                 np.asarray(c["lens"], np.int64)):
        got = _lens_call(name, wav, lens)
        assert all(_same_bits(g, w) for g, w in zip(got, want)), type(lens)
    # device lengths are clamped to [0, N] by the kernel (never read on the host)
    over = torch.tensor([513, 767, 768, 5000, 512, -7], dtype=torch.int32, device="cuda")
    got = _lens_call(name, wav, over)
    assert all(_same_bits(g, w) for g, w in zip(got, want))


def test_graph_follows_lengths_changed_in_place():
    import visual_onoma_to_wave_amd  # noqa: F401  (before the first GPU call, as GraphedSynthesis requires)
    name = "centred"
    c = R.CASES[name]
    wav = torch.from_numpy(R.signals(name).copy()).cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    _lens_call(name, wav, lens, prealloc=False)  # warm outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout = _lens_call(name, wav, lens, prealloc=False)
    for perm in ((0, 1, 2, 3, 4, 5), (3, 5, 0, 4, 2, 1), (2, 3, 1, 0, 5, 4)):
        new = [c["lens"][i] for i in perm]
        lens.copy_(torch.tensor(new, dtype=torch.int32, device="cuda"))
        graph.replay()
        want = _lens_call(name, wav, lens.clone())
        torch.cuda.synchronize()
        assert all(_same_bits(g, w) for g, w in zip(gout, want)), perm
        assert gout[3].tolist() == [c["frames"][i] for i in perm]


def test_refusals():
    from visual_onoma_to_wave_amd import ops
    name = "centred"
    c = R.CASES[name]
    wav = torch.from_numpy(R.signals(name).copy()).cuda()
    win, fb = _operands(name)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="mel_layout=2"):
        ops.stft_mel_lens(wav, win, fb, lens, channels_last=2)
    short = wav[:, :512].contiguous()  # N = pad: the dense entry refuses it, and so does this one
    with pytest.raises(RuntimeError, match="reflect padding needs N"):
        ops.stft_mel_ex(short, win, fb)
    with pytest.raises(RuntimeError, match="reflect padding needs N"):
        ops.stft_mel_lens(short, win, fb, lens)
    with pytest.raises(RuntimeError, match="power of two"):
        ops.stft_mel_lens(wav, win, fb, lens, n_fft=1000, pad=500)
    with pytest.raises(ValueError, match="shape"):
        ops.stft_mel_lens(wav, win, fb, lens[:5])
    with pytest.raises(ValueError, match="shape"):
        ops.stft_mel_lens(wav, win, fb, lens[None])
    with pytest.raises(ValueError, match="int32 / int64"):
        ops.stft_mel_lens(wav, win, fb, lens.float())
    with pytest.raises(ValueError, match="int32 / int64"):
        ops.stft_mel_lens(wav, win, fb, lens.to(torch.int16))
    with pytest.raises(ValueError, match="is on cpu"):
        ops.stft_mel_lens(wav, win, fb, lens.cpu())
    with pytest.raises(ValueError, match=r"in \[0, 2048\]"):
        ops.stft_mel_lens(wav, win, fb, [513, 767, 768, 2049, 512, 0])
    with pytest.raises(ValueError, match=r"in \[0, 2048\]"):
        ops.stft_mel_lens(wav, win, fb, [513, 767, 768])
    with pytest.raises(ValueError, match="mel must be fp32"):
        ops.stft_mel_lens(wav, win, fb, lens, mel=_nan(6, 80, 8))


def test_mel_spectrogram_lengths():
    from visual_onoma_to_wave_amd.audio import MelSpectrogram
    c = R.CASES["centred"]
    wav = torch.from_numpy(R.poisoned("centred")).cuda()
    m = MelSpectrogram()
    lens = torch.tensor(c["lens"], dtype=torch.int64, device="cuda")
    mel, energy, frames = m(wav, lens)
    cl, _, _ = m(wav, lens, channels_last=True)
    assert frames.tolist() == c["frames"] and _same_bits(cl.transpose(1, 2), mel)
    for b, (n, Fb) in enumerate(zip(c["lens"], c["frames"])):
        assert float(mel[b, :, Fb:].abs().sum()) == 0.0 and float(energy[b, Fb:].abs().sum()) == 0.0
        if Fb:
            d_mel, d_e = m(wav[b, :n])  # the utterance alone, through the dense entry
            assert _same_bits(mel[b, :, :Fb], d_mel) and _same_bits(energy[b, :Fb], d_e)
    one = m(wav[1], [767])  # 1-D waveform: squeezed like the dense call
    assert one[0].shape == (80, 9) and int(one[2]) == 3 and _same_bits(one[0], mel[1])


def test_tacotron_stft_lengths():
    from visual_onoma_to_wave_amd.audio import TacotronSTFT
    c = R.CASES["centred"]
    clean = np.clip(R.signals("centred"), -1, 1)
    wav = torch.from_numpy(clean).cuda()
    bad = wav.clone()
    for b, n in enumerate(c["lens"]):
        bad[b, n:] = float("nan")  # also out of [-1, 1]: the ragged path makes no host-side range check
    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    mel, energy, frames = stft.mel_spectrogram(bad, c["lens"])
    assert frames.tolist() == c["frames"] and not torch.isnan(mel).any()
    for b, (n, Fb) in enumerate(zip(c["lens"], c["frames"])):
        assert float(mel[b, :, Fb:].abs().sum()) == 0.0
        if Fb:
            d_mel, d_e = stft.mel_spectrogram(wav[b:b + 1, :n].contiguous())
            assert _same_bits(mel[b:b + 1, :, :Fb], d_mel) and _same_bits(energy[b:b + 1, :Fb], d_e)


# ------------------------------------------------------------------------------- win_length < filter_length

def test_mel_spectrogram_win_length_vs_oracle():
    from visual_onoma_to_wave_amd.audio import MelSpectrogram, get_spec
    wav = _wav(2, 3000, seed=800)
    logmel, energy = MelSpectrogram(1024, 200, win_length=800)(torch.from_numpy(wav).cuda())
    ref = [M.get_spec(torch.from_numpy(w), 1024, 200, 800) for w in wav]
    assert logmel.shape == (2, 80, 16)
    _check(logmel, energy, torch.stack([r[0] for r in ref]), torch.stack([r[1] for r in ref]))
    cfg = dict(audio=dict(stft=dict(filter_length=1024, hop_length=200, win_length=800)))
    g_mel, g_e = get_spec(torch.from_numpy(wav[0]).cuda(), cfg)  # get_spec reads stft.win_length
    assert _same_bits(g_mel, logmel[0]) and _same_bits(g_e, energy[0])


def test_tacotron_stft_win_length_vs_oracle():
    from visual_onoma_to_wave_amd.audio import TacotronSTFT
    wav = np.clip(_wav(2, 4001, seed=801), -1, 1)
    stft = TacotronSTFT(1024, 256, 800, 80, 22050, 0.0, 8000.0).cuda()
    mel, energy = stft.mel_spectrogram(torch.from_numpy(wav).cuda())
    mag = M.magnitude(torch.from_numpy(wav), 1024, 256, 800)  # the oracle's tacotron_mel composition, win = 800
    basis = torch.from_numpy(M.librosa_mel(22050, 1024, 80, 0.0, 8000.0))
    _check(mel, energy, torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5)),
           torch.linalg.vector_norm(mag, dim=-2))


def test_win_length_vs_reference_stft():
    """The kernels with the padded 800-sample window against the reference's own STFT.transform
    (tests/golden/make_goldens_win.py): vo_stft_mag's magnitude at test_mel.py's rel-L2 1e-5, and the mel kernel's
    frame energy (the L2 norm of the same |X|) at its energy bar."""
    from helpers import golden, rel_l2
    from visual_onoma_to_wave_amd import ops
    from visual_onoma_to_wave_amd.audio import MelSpectrogram, padded_window
    g = golden("stft_ref_win800")
    wav = torch.from_numpy(g["wav"]).cuda()
    mag = ops.stft_mag(wav, padded_window(800, 1024).cuda(), 1024, 256, eps=0.0).transpose(1, 2).cpu().numpy()
    assert mag.shape == g["magnitude"].shape
    assert rel_l2(mag, g["magnitude"]) < 1e-5
    _, energy = MelSpectrogram(1024, 256, win_length=800)(wav)
    np.testing.assert_allclose(energy.cpu().numpy(), np.linalg.norm(g["magnitude"].astype(np.float64), axis=1),
                               rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------- FeatureExtractor.process

UTT_LENS = [600, 1111, 1536, 2048]                                       # 3, 5, 7, 9 frames
UTT_DURS = [[1, 1, 1], [2, 0, 1, 2], [3, 1, 2, 1], [2, 2, 1, 3, 1]]     # a zero-length span: its kurtosis is NaN


def _utterances():
    w = _wav(4, 2048, seed=77)
    return [w[i, :n].copy() for i, n in enumerate(UTT_LENS)]


def _same_features(a, b):
    return all(x[k].shape == y[k].shape and x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes()
               for x, y in zip(a, b) for k in ("mel", "energy", "kurtosis")) and len(a) == len(b)


def test_process_one_launch_per_call(monkeypatch):
    from helpers import configs
    from visual_onoma_to_wave_amd import ops
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    wavs = _utterances()
    fx = FeatureExtractor(configs()[0])
    singles = [fx.process([w], [d])[0] for w, d in zip(wavs, UTT_DURS)]
    calls = dict(stft=0, char=0)

    def counted(fn, key):
        def wrapper(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(ops, "stft_mel_lens", counted(ops.stft_mel_lens, "stft"))
    monkeypatch.setattr(ops, "char_features", counted(ops.char_features, "char"))
    batch = fx.process(wavs, UTT_DURS)
    assert calls == dict(stft=1, char=1)
    assert _same_features(batch, singles)
    for o, d in zip(batch, UTT_DURS):
        assert o["mel"].shape == (sum(d), 80) and o["energy"].shape == (len(d),) and o["kurtosis"].dtype == np.float64
        assert np.isfinite(o["mel"]).all() and np.isfinite(o["energy"]).all()
    assert np.isnan(batch[1]["kurtosis"][1]) and np.isfinite(np.delete(batch[1]["kurtosis"], 1)).all()
    # B * N_max over max_batch_samples: [600, 1111] and [1536, 2048], the same results from two launches
    calls.update(stft=0, char=0)
    split = FeatureExtractor(configs()[0], max_batch_samples=4200).process(wavs, UTT_DURS)
    assert calls == dict(stft=2, char=2)
    assert _same_features(split, singles)
