"""The host side of the vocoder's segment sampler (visual_onoma_to_wave_amd/hifigan/data.py, DeviceCorpus.attach_waves;
DESIGN.md section 16) against the numpy model of tests/segment_check.py and the published Philox known answers.  No
GPU: the corpus of the refusal tests is packed into host memory."""

import numpy as np
import pytest

import segment_check as C


def _data():
    from visual_onoma_to_wave_amd.hifigan import data
    return data


@pytest.mark.parametrize("ctr, key, want", C.PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    assert C.philox(ctr, key) == want
    assert tuple(_data().philox4x32_10(ctr, key)) == want


def test_plan_host_known_answer():
    """counter 0, seed 0: w = 0x6627e8d5, so a span of 2^16 gives its upper half and a span of 1 gives 0."""
    D = _data()
    assert D.segment_plan_host([0, 1], 0, 0, 1, 4, [4 + 2 ** 16 - 1, 4]).tolist() == [[0, 0x6627]]
    assert D.segment_plan_host([1, 0], 0, 0, 1, 4, [4 + 2 ** 16 - 1, 4]).tolist() == [[1, 0]]


N_FRAMES = [1, 3, 4, 5, 14, 40, 10]  # below, at and above fps = 4; 10: span 7


@pytest.mark.parametrize("order", [[4], [4, 0, 6, 2, 5], [3, 1, 7, -1, 5]])  # n_order 1 and 5; ids outside the corpus
@pytest.mark.parametrize("counter", [0, 3, 2 ** 32 + 5, 2 ** 40 - 2])        # wraps order; above 2^32
@pytest.mark.parametrize("seed", [0, 1234, 2 ** 64 - 1])
def test_plan_host_matches_the_model(order, counter, seed):
    D = _data()
    B, fps = 13, 4
    got = D.segment_plan_host(order, counter, seed, B, fps, N_FRAMES)
    want = C.model_plan(order, counter, seed, B, fps, N_FRAMES)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for src, start in got.tolist():
        if 0 <= src < len(N_FRAMES):
            assert 0 <= start <= max(N_FRAMES[src] - fps, 0)
        else:
            assert start == 0
    # the draw is a function of the row's number alone: two calls of 13 rows are one of 26
    both = D.segment_plan_host(order, counter, seed, 2 * B, fps, N_FRAMES)
    assert np.array_equal(both[:B], got)
    assert np.array_equal(both[B:], D.segment_plan_host(order, counter + B, seed, B, fps, N_FRAMES))


def test_every_start_of_a_span_is_drawn():
    plan = _data().segment_plan_host([6], 0, 7, 4096, 4, N_FRAMES)  # F = 10, fps = 4: span 7
    assert sorted(set(plan[:, 1].tolist())) == list(range(7))
    assert np.array_equal(plan, C.model_plan([6], 0, 7, 4096, 4, N_FRAMES))


def test_check_segment_plan():
    D = _data()
    ok = [(0, 0), (4, 10), (3, 1), (1, 0)]
    got = D.check_segment_plan(ok, N_FRAMES, 4)
    assert got.dtype == np.int32 and got.tolist() == [list(r) for r in ok]
    for bad, msg in [((-1, 0), r"row 2: src -1 is outside \[0, 7\)"),
                     ((7, 0), r"row 2: src 7 is outside \[0, 7\)"),
                     ((4, -1), r"row 2: start -1 is outside \[0, max\(F - fps, 0\)\] = \[0, 10\]"),
                     ((4, 11), r"row 2: start 11 is outside \[0, max\(F - fps, 0\)\] = \[0, 10\]"),
                     ((1, 1), r"row 2: start 1 is outside \[0, max\(F - fps, 0\)\] = \[0, 0\]")]:
        with pytest.raises(ValueError, match=msg):
            D.check_segment_plan(ok[:2] + [bad] + ok[2:], N_FRAMES, 4)
    with pytest.raises(ValueError, match=r"shape \(B, 2\)"):
        D.check_segment_plan([(0, 0, 0)], N_FRAMES, 4)
    with pytest.raises(ValueError, match=r"shape \(B, 2\)"):
        D.check_segment_plan(np.zeros((1, 2), np.float32), N_FRAMES, 4)


def test_attach_waves_refusals():
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    hop = 8
    mels, wavs = C.make([3, 5, 2], [24, 40, 16], 5, "int16", 0)
    corpus = DeviceCorpus.from_arrays(C.utterances(mels), 4, 1, "cpu")
    assert corpus.waves is None

    def refused(w, msg, **kw):
        with pytest.raises(ValueError, match=msg):
            corpus.attach_waves(w, hop, **kw)
        assert corpus.waves is None
    refused(wavs[:2], "2 waveforms for 3 utterances")
    refused([wavs[0], wavs[1].reshape(2, 20), wavs[2]], r"utterance 1 \('u1'\): the waveform has shape \(2, 20\)")
    refused([wavs[0], wavs[1], wavs[2][:0]], r"utterance 2 \('u2'\): the waveform has shape \(0,\)")
    refused([wavs[0], wavs[1].astype(np.float32), wavs[2]], r"utterance 1 \('u1'\): the waveform is float32, the ones "
                                                            "before it are int16")
    refused([w.astype(np.float64) for w in wavs[:2]] + [wavs[2]], r"utterance 2 \('u2'\): the waveform is int16, the "
                                                                  "ones before it are floating point")
    refused([w.astype(np.int32) for w in wavs], r"utterance 0 \('u0'\): the waveform is int32")
    # 1 + N // hop >= F: 31 samples are 4 frames, the mel has 5; 32 are enough
    refused([wavs[0], wavs[1][:31], wavs[2]], r"utterance 1 \('u1'\): 31 samples are 1 \+ N // hop = 4 frames at hop 8, "
                                              "the mel has 5")
    refused(wavs, "max_wav_value", max_wav_value=0.0)
    with pytest.raises(ValueError, match="hop must be >= 1"):
        corpus.attach_waves(wavs, 0)
    corpus.attach_waves([wavs[0], wavs[1][:32], wavs[2][:9]], hop)
    assert corpus.waves.U == 3 and corpus.waves.is_int16 == 1 and corpus.waves.max_wav_value == 32768.0
    assert corpus.n_samples == [24, 32, 9] and corpus.wave_hop == hop
    assert corpus.wave_tensors["sample_off"].tolist() == [0, 24, 56, 72]  # every utterance at a multiple of 8
    flat = corpus.wave_tensors["wav"].numpy()
    assert flat.dtype == np.int16 and np.array_equal(flat[56:65], wavs[2][:9]) and not flat[65:].any()
    corpus.attach_waves([w.astype(np.float64) / 3 for w in wavs], hop)  # floating point is kept as fp32
    assert corpus.waves.is_int16 == 0 and corpus.wave_tensors["wav"].dtype.is_floating_point
    assert np.array_equal(corpus.wave_tensors["wav"].numpy()[:24], (wavs[0].astype(np.float64) / 3).astype(np.float32))


def test_sampler_refusals():
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    from visual_onoma_to_wave_amd.hifigan import SegmentSampler
    mels, wavs = C.make([3, 5], [24, 40], 5, "float32", 1)
    corpus = DeviceCorpus.from_arrays(C.utterances(mels), 4, 1, "cpu")
    with pytest.raises(ValueError, match="no waveforms"):
        SegmentSampler(corpus, 32, 8, 2)
    corpus.attach_waves(wavs, 8)
    with pytest.raises(ValueError, match="segment_size 33 is not a multiple of hop 8"):
        SegmentSampler(corpus, 33, 8, 2)
    with pytest.raises(ValueError, match="attached with hop 8"):
        SegmentSampler(corpus, 32, 4, 2)
    with pytest.raises(ValueError, match="mel must be"):
        SegmentSampler(corpus, 32, 8, 2, mel="gta")
    s = SegmentSampler(corpus, 32, 8, 3)
    assert s.fps == 4 and s.epoch_steps == 1 and s.position() == 0 and s.order.tolist() == [0, 1]
    assert s.seek(2 ** 33 + 1).position() == 2 ** 33 + 1
    order = s.order
    assert s.set_order([1, 0]).order is order and order.tolist() == [1, 0]
    for bad in ([0], [0, 2], [0.0, 1.0]):
        with pytest.raises(ValueError, match="set_order"):
            s.set_order(bad)
    with pytest.raises(ValueError, match="seek"):
        s.seek(-1)
