"""Host side of the ragged mel front end (no GPU): the frame-count rule, the zero-padded window of
win_length < filter_length, the batch padding, and the float64 reference of ``mel_ragged_check`` pinned to
``oracle.mel`` -- under ``test_mel.py``'s bars -- before ``test_gpu_mel_ragged.py`` judges the kernel by it."""

import copy

import numpy as np
import pytest
import torch

import mel_ragged_check as R
from helpers import configs
from oracle import mel as M
from test_mel import _check

FRAMINGS = [(1024, 256, 512), (1024, 256, 384)]  # torchaudio center=True; HiFi-GAN's (n_fft - hop) / 2


@pytest.mark.parametrize("n_fft,hop,pad", FRAMINGS)
def test_frames_rule(n_fft, hop, pad):
    from visual_onoma_to_wave_amd import ops
    for n in range(0, 2101):
        F = ops.stft_mel_frames(n, n_fft, hop, pad)
        assert F == R.closed_form_frames(n, n_fft, hop, pad), n
        if n > pad:  # torch can reflect-pad it: its own frame count
            x = torch.zeros(1, n)
            if pad == n_fft // 2:
                X = torch.stft(x, n_fft, hop_length=hop, window=torch.ones(n_fft), center=True, pad_mode="reflect",
                               return_complex=True)
            else:
                xp = torch.nn.functional.pad(x[:, None], (pad, pad), mode="reflect")[:, 0]
                X = torch.stft(xp, n_fft, hop_length=hop, window=torch.ones(n_fft), center=False,
                               return_complex=True)
            assert F == X.shape[-1], n
        else:
            assert F == 0, n


def test_frames_rule_default_pad_and_bad_sizes():
    from visual_onoma_to_wave_amd import ops
    assert ops.stft_mel_frames(2048) == 9 and ops.stft_mel_frames(512) == 0
    assert ops.stft_mel_frames(100, 64, 16) == 1 + 100 // 16
    assert ops.stft_mel_frames(2048, 1024, 0, 512) == 0 and ops.stft_mel_frames(-5, 1024, 256, 512) == 0


@pytest.mark.parametrize("win", [800, 1023, 2, 1024])
def test_padded_window_is_torch_stft_placement(win):
    from visual_onoma_to_wave_amd.audio import padded_window
    n_fft, hop = 1024, 256
    w = padded_window(win, n_fft)
    assert w.shape == (n_fft,) and w.dtype == torch.float32
    left = (n_fft - win) // 2
    assert torch.equal(w[left:left + win], torch.hann_window(win, periodic=True))
    assert float(w[:left].abs().sum()) == 0.0 and float(w[left + win:].abs().sum()) == 0.0
    x = torch.from_numpy(np.random.default_rng(win).standard_normal((2, 3000)))
    a = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True).double(),
                   center=True, pad_mode="reflect", return_complex=True)
    b = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w.double(), center=True, pad_mode="reflect",
                   return_complex=True)
    torch.testing.assert_close(a, b, rtol=0.0, atol=1e-12)


def test_padded_window_refuses_a_longer_window():
    from visual_onoma_to_wave_amd.audio import padded_window
    with pytest.raises(ValueError, match="win_length"):
        padded_window(1025, 1024)
    assert torch.equal(padded_window(1024, 1024), torch.hann_window(1024, periodic=True))


def test_pad_waves():
    from visual_onoma_to_wave_amd.audio import pad_waves
    rng = np.random.default_rng(0)
    wavs = [rng.standard_normal(n) for n in (7, 31, 0, 19)]
    wav, lens = pad_waves(wavs)
    assert wav.shape == (4, 31) and wav.dtype == torch.float32 and not wav.is_cuda
    assert lens.dtype == torch.int32 and lens.tolist() == [7, 31, 0, 19]
    for b, w in enumerate(wavs):
        assert np.array_equal(wav[b, :len(w)].numpy(), w.astype(np.float32))
        assert float(wav[b, len(w):].abs().sum()) == 0.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_table_is_the_closed_form(name):
    c = R.CASES[name]
    assert [R.closed_form_frames(n, c["n_fft"], c["hop"], c["pad"]) for n in c["lens"]] == c["frames"]
    assert max(c["frames"]) == R.capacity(c)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_pinned_to_oracle(name):
    """Every row of the GPU case table: the float64 reference against oracle.mel (torch.stft), _check's bars."""
    c = R.CASES[name]
    wav, fb = R.signals(name), R.filterbank(name)
    for b, (n, Fb) in enumerate(zip(c["lens"], c["frames"])):
        mel, energy, fstats = R.reference(name)[b]
        assert mel.shape == (c["n_mels"], Fb) and energy.shape == (Fb,) and fstats.shape == (Fb, 2)
        if Fb == 0:
            continue
        x = torch.from_numpy(wav[b, :n].copy())
        if c["pad"] == c["n_fft"] // 2:
            o_mel, o_e = M.get_spec(x, c["n_fft"], c["hop"], c["n_fft"], c["n_mels"])
        else:
            # the HiFi-GAN framing through the oracle's centred magnitude: pad by 384 first; n_fft / 2 = 2 hops, so
            # centred frame f + 2 of the padded signal is frame f of this framing (and touches no centre padding)
            assert c["n_fft"] // 2 == 2 * c["hop"] and not c["clip"]
            xp = torch.nn.functional.pad(x[None, None], (c["pad"], c["pad"]), mode="reflect")[0, 0]
            mag = M.magnitude(xp, c["n_fft"], c["hop"], c["n_fft"])[:, 2:2 + Fb].double()
            o_mel = torch.log(torch.clamp_min(fb.double().t() @ mag, R.LOG_FLOOR)).float()
            o_e = torch.linalg.vector_norm(mag, dim=0).float()
        assert o_mel.shape == mel.shape
        _check(torch.from_numpy(mel), torch.from_numpy(energy), o_mel, o_e)
        # the statistics are sums over the same |X|: the first is the squared energy
        np.testing.assert_allclose(fstats[:, 0], energy ** 2, rtol=1e-12)


def test_oracle_and_window_pinned_to_reference_win800():
    """win_length 800 in filter_length 1024 against the reference's own STFT.transform
    (tests/golden/make_goldens_win.py): its padded window is padded_window's, and the oracle's |STFT| with
    win=800 is its magnitude at test_mel.py's rel-L2 bar."""
    from helpers import golden, rel_l2
    from visual_onoma_to_wave_amd.audio import padded_window
    g = golden("stft_ref_win800")
    np.testing.assert_allclose(g["window"], padded_window(800, 1024).numpy(), atol=5e-7)
    assert float(np.abs(g["window"][:112]).sum()) == 0.0 and float(np.abs(g["window"][912:]).sum()) == 0.0
    mag = M.magnitude(torch.from_numpy(g["wav"]), 1024, 256, 800).numpy()
    assert mag.shape == g["magnitude"].shape == (2, 513, 16)
    assert rel_l2(mag, g["magnitude"]) < 1e-5


def test_win_length_constructs():
    from visual_onoma_to_wave_amd.audio import TacotronSTFT, padded_window
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    st = TacotronSTFT(1024, 256, 800, 80, 22050, 0.0, 8000.0)
    assert torch.equal(st._mel.window, padded_window(800, 1024))
    with pytest.raises(ValueError, match="win_length"):
        TacotronSTFT(1024, 256, 1100, 80, 22050, 0.0, 8000.0)
    cfg = copy.deepcopy(configs()[0])
    cfg["audio"]["stft"]["win_length"] = 800
    fx = FeatureExtractor(cfg, device="cpu")
    assert torch.equal(fx.window, padded_window(800, 1024))
    assert torch.equal(FeatureExtractor(configs()[0], device="cpu").window, torch.hann_window(1024, periodic=True))


def test_process_refuses_durations_past_the_signal():
    """sum(durations) > the utterance's own frame count: a ValueError naming it, raised on the host before anything
    is launched (the extractor lives on the CPU here, where a launch would raise RuntimeError instead)."""
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    fx = FeatureExtractor(configs()[0], device="cpu")
    wavs = [np.zeros(2048, np.float32), np.zeros(600, np.float32)]  # 9 and 3 frames
    with pytest.raises(ValueError, match=r"utterance 1\b.*4 frames.*600 samples give 3"):
        fx.process(wavs, [[4, 5], [2, 2]])
    with pytest.raises(ValueError, match=r"utterance 0\b"):
        fx.process(wavs, [[4, 6], [2, 1]])


def test_chunks_respect_max_batch_samples():
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    fx = FeatureExtractor(configs()[0], device="cpu", max_batch_samples=4096)
    lens = [600, 2048, 1000, 1500, 5000, 100]
    runs = fx._chunks(lens)
    assert [i for r in runs for i in r] == list(range(len(lens)))
    for r in runs:
        assert len(r) == 1 or len(r) * max(lens[i] for i in r) <= 4096
    assert runs == [[0, 1], [2, 3], [4], [5]]
    assert FeatureExtractor(configs()[0], device="cpu")._chunks(lens) == [list(range(len(lens)))]
