"""The request sets of tests/test_gpu_graphed_synthesis.py and the oracle's waveforms for the first of them, shared
with the CPU self-test of the PCM checker (tests/test_pcm_check.py verifies pcm_check's band cap on exactly these
waveforms).  Everything is computed once per process and never changed."""

import functools

import numpy as np
import torch

from helpers import hifigan_arrays, hifigan_h, stats, vtts_arrays

BATCH, MAX_SRC, CAP = 3, 7, 64
HOP = 256
DUR_BIAS_SHIFT = 1.6  # synthetic weights predict zero durations without it (the goldens' shift)
DUR_KEY = "variance_adaptor.duration_predictor.linear_layer.bias"
PCM_SCALE = 32768.0


def request_set(i):
    """Request set i (0, 1, 2): dict of numpy inputs for BATCH requests of MAX_SRC characters, and the controls in
    three of the shapes ``ops.control_view`` accepts.  Set 0 is the control tests' oracle case (its rounding and
    bucketize margins are asserted there)."""
    from visual_onoma_to_wave_amd import synth
    b = synth.acoustic_batch((300, 411, 522)[i], BATCH, MAX_SRC, 20, ragged=True)
    rng = np.random.default_rng(i)
    if i == 0:
        ec = rng.uniform(0.5, 1.6, size=(BATCH, MAX_SRC)).astype(np.float32)
        dc = rng.uniform(0.0, 2.5, size=(BATCH, MAX_SRC)).astype(np.float32) * np.float32(0.5)  # 35 / 35 / 36 frames
    elif i == 1:
        ec = rng.uniform(0.7, 1.3, size=(BATCH, 1)).astype(np.float32)
        dc = rng.uniform(0.4, 1.8, size=(MAX_SRC,)).astype(np.float32)
    else:
        ec, dc = None, np.float32(1.5)
    return dict(audiotypes=b["audiotypes"], texts=b["texts"], src_lens=b["src_lens"], images=b["images"],
                e_control=ec, d_control=dc)


@functools.lru_cache(maxsize=None)
def oracle_set0():
    """The oracle on request set 0 with CAP as the mel capacity: (mel_len (B,), [waveform of utterance b on the
    oracle's own mel[b, :mel_len[b]], fp32 (N_b,)]).

    The mel of an utterance depends on the padded length (PostNet's convs are not masked: its last ten frames see
    what follows them), so the oracle has to pad to CAP as the model under test does.  The reference cannot do that
    free-running (its mask is then built for the longest utterance, not for max_len), so the oracle runs twice: free
    to predict the durations, then with those durations as ``d_targets`` and mel_lens / max_mel_len = CAP, which
    builds the mask at CAP and pads the length regulator's output to it (``pad(output, max_len)``); the energy path
    is the predicted one both times."""
    from oracle import acoustic as A
    from oracle import vocoder as V
    torch.set_num_threads(16)
    r = request_set(0)
    sd = A.complete_state_dict(vtts_arrays(), stats()["energy"])
    sd[DUR_KEY] = sd[DUR_KEY] + DUR_BIAS_SHIFT
    t = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    gsd = V.fold_weight_norm({k: torch.from_numpy(np.array(v)) for k, v in hifigan_arrays().items()})
    args = (sd, t(r["audiotypes"]), t(r["texts"]), t(r["src_lens"]), MAX_SRC)
    kw = dict(images=t(r["images"]), energy_stats=stats()["energy"], e_control=t(r["e_control"]))
    with torch.no_grad():
        free = A.vtts_forward(*args, d_control=t(r["d_control"]), **kw)
        mel_len = free[9].numpy().astype(np.int64)
        assert 0 < mel_len.min() and mel_len.max() <= CAP and len(set(mel_len.tolist())) > 1, mel_len
        out = A.vtts_forward(*args, mels=torch.zeros(BATCH, CAP, 80), mel_lens=free[9], max_mel_len=CAP,
                             d_targets=free[5], **kw)
        assert out[1].shape == (BATCH, CAP, 80) and out[9].tolist() == mel_len.tolist()
        waves = []
        for b in range(BATCH):
            m1 = out[1][b:b + 1, :int(mel_len[b])].transpose(1, 2).contiguous()
            waves.append(V.generator(gsd, m1, hifigan_h()).reshape(-1).numpy())
    return mel_len, waves


def infer_mels():
    """The (B, T, 80) mel batch of test_gpu_ragged_generator.py (its ``mel`` fixture) and its LENGTHS."""
    import test_gpu_ragged_generator as R
    g = torch.Generator().manual_seed(4023)
    return torch.randn(R.B, R.T, 80, generator=g) * 1.5 - 4.0, R.LENGTHS


@functools.lru_cache(maxsize=None)
def oracle_infer_waves():
    """The fp32 oracle generator on each utterance of ``infer_mels`` alone (None for an empty one)."""
    from oracle import vocoder as V
    torch.set_num_threads(16)
    mel, lengths = infer_mels()
    gsd = V.fold_weight_norm({k: torch.from_numpy(np.array(v)) for k, v in hifigan_arrays().items()})
    with torch.no_grad():
        return [V.generator(gsd, mel[b:b + 1, :n].transpose(1, 2).contiguous(), hifigan_h()).reshape(-1).numpy()
                if n else None for b, n in enumerate(lengths)]
