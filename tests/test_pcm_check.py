"""CPU self-test of the PCM checker (tests/pcm_check.py).  Accept: the store emulated on the CPU passes on the
waveforms the GPU tests use -- the fp32 oracle generator on the same seeded mels and requests -- and those waveforms
alone meet the band cap.  Reject: each deliberate fault raises."""

import numpy as np
import pytest

import graphed_case as G
import pcm_check as PC
import test_gpu_conv_post_pcm as M

SCALES = M.SCALES


def _padded(waves):
    """[(N_b,) or None] -> ((B, T) fp32 with zeros past each utterance, rows)."""
    rows = [0 if w is None else len(w) for w in waves]
    y = np.zeros((len(waves), max(rows) + 256), np.float32)  # a padded frame after the longest utterance
    for b, w in enumerate(waves):
        if w is not None:
            y[b, :len(w)] = w
    return y, rows


@pytest.fixture(scope="module", params=["infer_mels", "request_set0"])
def wave(request):
    return _padded(G.oracle_infer_waves() if request.param == "infer_mels" else G.oracle_set0()[1])


def test_expected_pcm_is_the_host_cast_in_range_and_saturates_outside():
    y = np.array([[0.0, 0.5, -0.5, 0.99996, -0.99996, 3.1e-5, -3.1e-5, 6.2e-5, -6.2e-5, 0.25001, -0.7503]], np.float32)
    for scale in SCALES:
        np.testing.assert_array_equal(PC.expected_pcm(y, scale), (y * scale).astype("int16"))
    assert PC.expected_pcm(np.float32([3.1e-5, -3.1e-5]), 32768.0).tolist() == [1, -1]  # toward zero, not floor
    assert PC.expected_pcm(np.float32([1.9 / 32768, -1.9 / 32768]), 32768.0).tolist() == [1, -1]
    edge = np.float32([1.0, -1.0, np.nan, np.inf, -np.inf, 1.5])
    assert PC.expected_pcm(edge, 32768.0).tolist() == [32767, -32768, 0, 32767, -32768, 32767]
    assert PC.expected_pcm(edge, 32767.0).tolist() == [32767, -32767, 0, 32767, -32768, 32767]
    # the product is formed in fp32: 32767 is no power of two, the fp64 product truncates differently somewhere
    y = np.random.default_rng(0).uniform(-1, 1, 200000).astype(np.float32)
    f64 = np.trunc(y.astype(np.float64) * 32767.0).astype(np.int16)
    assert (PC.expected_pcm(y, 32767.0) != f64).any()
    assert (PC.expected_pcm(y, 32768.0) == np.trunc(y.astype(np.float64) * 32768.0).astype(np.int16)).all()


@pytest.mark.parametrize("scale", SCALES)
def test_oracle_waveforms_meet_the_band_cap(wave, scale):
    y, rows = wave
    assert len(set(rows)) > 1 and np.abs(y).max() * scale < 32768
    frac = PC.check_pcm(PC.emulate(y, scale, rows), y, scale, rows)
    valid = np.arange(y.shape[1])[None, :] < np.asarray(rows)[:, None]
    print(f"band fraction {frac:.4f}; peak |y| {np.abs(y).max():.4f}, rms {np.sqrt((y[valid] ** 2).mean()):.4f}")
    assert 0 < frac <= PC.BAND_CAP
    # a last-bit difference of the reference moves no sample outside the band and none by more than one step
    for nudge in (np.float32(-np.inf), np.float32(np.inf)):
        PC.check_pcm(PC.emulate(np.nextafter(y, nudge), scale, rows), y, scale, rows)


@pytest.mark.parametrize("mutate", PC.MUTATIONS)
def test_checker_rejects_mutation(wave, mutate):
    y, rows = wave
    y = y.copy()
    y[0, [5, 300, 301]] = 1.0  # three saturated samples: the wrap lands on -32768
    PC.check_pcm(PC.emulate(y, 32768.0, rows), y, 32768.0, rows)
    with pytest.raises(AssertionError):
        PC.check_pcm(PC.emulate(y, 32768.0, rows, mutate), y, 32768.0, rows)


def test_checker_rejects_a_reference_on_integers():
    """Silence or a saturated waveform cannot pass by exclusion: the band cap itself fails."""
    y = np.zeros((2, 300), np.float32)
    with pytest.raises(AssertionError, match="cap"):
        PC.check_pcm(PC.emulate(y, 32768.0), y, 32768.0)
    y = np.ones((2, 300), np.float32)
    with pytest.raises(AssertionError, match="cap"):
        PC.check_pcm(PC.emulate(y, 32768.0), y, 32768.0)


@pytest.mark.parametrize("c", M.CASES + M.RAGGED, ids=[c["name"] for c in M.CASES + M.RAGGED])
def test_conv_post_operands_fill_the_range(c):
    """The operands of the GPU matrix: a float64 conv_post on them spreads over the int16 range and meets the cap."""
    for seed in (0, 1):
        x, w, bias = PC.post_operands(c, seed)
        y = PC.post_reference(x, w, bias).numpy()
        assert 0.9 < np.abs(y).max() < 1.0 and np.abs(y).mean() > 0.3
        for scale in SCALES:
            PC.check_pcm(PC.emulate(y, scale), y, scale, name=c["name"])


def test_matrix_coverage():
    have = {(c["dt"], c["C"], c["K"], c["T"]) for c in M.CASES}
    assert have >= {("bf16", 32, 7, T) for T in (249, 250, 251, 501)}
    for T in (255, 256, 257):
        assert have >= {("bf16", 32, 5, T), ("bf16", 64, 7, T), ("f32", 32, 7, T)}
    assert all(c["B"] == 3 for c in M.CASES + M.RAGGED) and PC.GUARD == 64 and PC.GUARD_VALUE == 0x5A5A
    assert M.SCALES == (32768.0, 32767.0)
