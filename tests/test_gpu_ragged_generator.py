"""The whole vocoder on a ragged batch: ``Generator.run(mel, lengths)``.

Row b of the ragged run must be what the utterance gives alone -- the oracle on mel[b, :, :len_b] -- followed by exact
zeros, with the padded mel frames holding NaN (nothing may read them).  The bars are those of
test_generator_long_vs_reference_golden (1e-4 in fp32, helpers.bf16_bar in bf16), on the whole utterance and, with the
bar computed on that same window, on its last R frames of samples: R is the receptive field that
tests/test_ragged_receptive_field.py pins, the only place a padded frame could reach, and a masking error of one row
there would vanish in a whole-signal norm.
"""

import numpy as np
import pytest
import torch

from helpers import bf16_bar, configs, hifigan_arrays, hifigan_h, oracle_generator_bf16, rel_l2, vtts_arrays
from test_ragged_receptive_field import HOP, R_FRAMES
from weights import load_into

pytestmark = pytest.mark.gpu

B, T = 4, 40
LENGTHS = (40, 23, 8, 0)


@pytest.fixture(scope="module")
def gen(device):
    from visual_onoma_to_wave_amd import hifigan
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    return g.to(device)


@pytest.fixture(scope="module")
def mel():
    """(B, T, 80) channels-last fp32 on the host, finite everywhere."""
    g = torch.Generator().manual_seed(4023)
    return torch.randn(B, T, 80, generator=g) * 1.5 - 4.0


@pytest.fixture(scope="module")
def oracle_refs(mel):
    """Per utterance: the oracle on its own frames, in fp32 and under bf16 autocast (computed once, never changed)."""
    from oracle import vocoder as V
    torch.set_num_threads(16)
    gsd = V.fold_weight_norm({k: torch.from_numpy(np.array(v)) for k, v in hifigan_arrays().items()})
    refs = []
    for b, n in enumerate(LENGTHS):
        if n == 0:
            refs.append(None)
            continue
        m1 = mel[b:b + 1, :n].transpose(1, 2).contiguous()
        with torch.no_grad():
            r32 = V.generator(gsd, m1, hifigan_h()).reshape(-1)
        refs.append((r32, oracle_generator_bf16(gsd, m1, hifigan_h()).reshape(-1)))
    return refs


def _padded(mel):
    m = mel.clone()
    for b, n in enumerate(LENGTHS):
        m[b, n:] = float("nan")
    return m.cuda()


@pytest.mark.parametrize("dt,as_tensor", [(torch.bfloat16, True), (torch.float32, False)])
def test_ragged_generator_vs_oracle(gen, mel, oracle_refs, dt, as_tensor):
    gen.set_compute_dtype(dt)
    lengths = torch.tensor(LENGTHS, dtype=torch.int64, device="cuda") if as_tensor else list(LENGTHS)
    with torch.no_grad():
        wav = gen.run(_padded(mel), lengths).cpu()
    assert wav.shape == (B, HOP * T) and torch.isfinite(wav).all()
    for b, n in enumerate(LENGTHS):
        assert (wav[b, HOP * n:] == 0).all(), f"utterance {b}: samples past {HOP * n} are not exactly 0"
        if n == 0:
            continue
        r32, r16 = oracle_refs[b]
        lo = HOP * max(n - R_FRAMES, 0)
        for name, sl in (("whole", slice(0, HOP * n)), (f"last {R_FRAMES} frames", slice(lo, HOP * n))):
            e = rel_l2(wav[b, sl], r32[sl])
            tol = 1e-4 if dt == torch.float32 else bf16_bar(r32[sl], r16[sl])
            print(f"{dt} utterance {b} ({n} frames) {name}: rel-L2 {e:.2e} (bar {tol:.2e})")
            assert e < tol, (b, name, e, tol)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_dense_path_unchanged_and_ragged_equals_single_utterances(gen, mel, oracle_refs, dt):
    """lengths=None is the path it was: the batch's rows against ``gen.run`` on the single utterances and against
    the oracle (utterance 0 is unpadded).  And the ragged rows against ``gen.run`` on the unpadded single utterances,
    under the same bar."""
    gen.set_compute_dtype(dt)
    r32, r16 = oracle_refs[0]
    tol = 1e-4 if dt == torch.float32 else bf16_bar(r32, r16)
    with torch.no_grad():
        dense = gen.run(mel.cuda()).cpu()
        singles = [gen.run(mel[b:b + 1].cuda()).cpu()[0] for b in range(B)]
        ragged = gen.run(_padded(mel), list(LENGTHS)).cpu()
        cut = [gen.run(mel[b:b + 1, :n].contiguous().cuda()).cpu()[0] if n else None for b, n in enumerate(LENGTHS)]
    assert rel_l2(dense[0], r32) < tol
    for b, n in enumerate(LENGTHS):
        assert torch.equal(dense[b], singles[b]) or rel_l2(dense[b], singles[b]) < tol
        if n:
            e = rel_l2(ragged[b, :HOP * n], cut[b])
            print(f"{dt} utterance {b}: ragged row vs run() on it alone: rel-L2 {e:.2e}")
            assert e < tol


def test_ragged_run_under_graph_follows_lengths_changed_in_place(gen, mel):
    """The lengths stay on the device: the ragged run is capturable, and a replay after an in-place change of the
    lengths tensor equals an eager call on the new lengths, bit for bit."""
    gen.set_compute_dtype(torch.bfloat16)
    static = mel.cuda()
    lens = torch.tensor(LENGTHS, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        gen.run(static, lens)  # warm the pack cache and the side streams outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gout = gen.run(static, lens)
        for perm in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)):
            lens.copy_(torch.tensor([LENGTHS[i] for i in perm], dtype=torch.int64, device="cuda"))
            graph.replay()
            want = gen.run(static, lens.clone())
            torch.cuda.synchronize()
            assert torch.equal(gout, want), perm
            for b, i in enumerate(perm):
                assert (gout[b, HOP * LENGTHS[i]:] == 0).all()


def test_synthesis_pipeline_ragged_matches_sequential(gen, device):
    """SynthesisPipeline(ragged=True) hands the acoustic model's device-side mel_len (out[9]) to the vocoder: batch
    for batch what the sequential model -> ``gen.run(out[1], out[9])`` gives."""
    from visual_onoma_to_wave_amd import synth
    from visual_onoma_to_wave_amd.model import vTTS
    from visual_onoma_to_wave_amd.pipeline import SynthesisPipeline
    vtts = vTTS(*configs())
    load_into(vtts, vtts_arrays())
    vtts = vtts.to(device).eval()
    vtts.set_precision("mixed")
    gen.set_compute_dtype(torch.bfloat16)
    batches = []
    for seed in (31, 32):
        b = synth.acoustic_batch(seed, 4, 12, 48, ragged=True)
        # teacher-forced durations cut per utterance, so that the model's mel_len (their row sums) is ragged
        d = np.minimum(b["d_targets"], np.array([[99.0], [3.0], [2.0], [1.0]], dtype=np.float32))
        b["d_targets"], b["mel_lens"] = d, d.sum(1).astype(np.float32)
        t = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        batches.append([t["audiotypes"], t["texts"], t["src_lens"], t["max_src_len"], t["mels"], t["mel_lens"],
                        t["max_mel_len"], None, None, t["d_targets"], t["images"], None, True])
    with torch.no_grad():
        ref = []
        for args in batches:
            out = vtts(*args)
            ref.append((out[9].cpu(), gen.run(out[1], out[9]).cpu()))
        pipe = SynthesisPipeline(vtts, gen, ragged=True)
        pipe.submit(*batches[0])
        got = []
        for i in range(len(batches)):
            if i + 1 < len(batches):
                pipe.submit(*batches[i + 1])
            got.append(pipe.next_wav()[1])
        torch.cuda.synchronize()
    for (mel_len, r), g in zip(ref, got):
        assert torch.equal(r, g.cpu())
        assert len(set(mel_len.tolist())) > 1, "the batch is not ragged"
        for b, n in enumerate(mel_len.tolist()):
            assert (r[b, HOP * int(n):] == 0).all() and torch.isfinite(r[b]).all()


def test_vocoder_infer_ragged_equals_per_utterance_calls(gen, mel):
    """utils.model.vocoder_infer(..., ragged=True) with lengths in samples, as the reference passes them: the same
    int16 arrays as one call per utterance on its own ceil(length / hop) frames."""
    from visual_onoma_to_wave_amd.utils.model import vocoder_infer
    pre, model_cfg, _ = configs()
    gen.set_compute_dtype(torch.bfloat16)
    samples = [40 * HOP, 23 * HOP - 100, 8 * HOP - 255, 300]
    mels = mel.transpose(1, 2).contiguous().cuda()  # (B, 80, T), as the reference's synthesis loop holds them
    got = vocoder_infer(mels, gen, model_cfg, pre, lengths=samples, ragged=True)
    assert [w.shape[0] for w in got] == samples and all(w.dtype == np.int16 for w in got)
    for b, n in enumerate(samples):
        frames = -(-n // HOP)
        alone = vocoder_infer(mels[b:b + 1, :, :frames].contiguous(), gen, model_cfg, pre, lengths=[n])
        np.testing.assert_array_equal(got[b], alone[0])
    with pytest.raises(ValueError):
        vocoder_infer(mels, gen, model_cfg, pre, ragged=True)
