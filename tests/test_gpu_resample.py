"""Sample-rate conversion on the GPU (vo_resample, ``ops.resample``, ``audio.Resample`` and its callers; DESIGN.md
section 17) against the float64 yardstick tests/resample_check.py, which tests/test_resample_cpu.py holds against
analytically sampled sines.  Tolerances are the yardstick's derived bound; impulses, the invariances, the graph replay
and the callers are compared by their bits."""

import ctypes

import numpy as np
import pytest
import torch

import pcm_check as PC
import resample_check as R
from visual_onoma_to_wave_amd.ops import RESAMPLE_TILE as TILE

pytestmark = pytest.mark.gpu

BIG = (320, 147)  # 48000 -> 22050


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(x, O, M, lens=None, skip=None, N_out=None, mwv=None, pcm=None):
    """``ops.resample`` of a numpy batch into a poisoned, guarded buffer -> (y (B, N_out), out_lens) as numpy."""
    from visual_onoma_to_wave_amd import ops
    B = x.shape[0]
    N_out = R.length(x.shape[1], O, M) if N_out is None else N_out
    buf = torch.from_numpy(R.guarded(B, N_out, np.int16 if pcm else np.float32)).cuda()
    out = buf[:B * N_out].view(B, N_out)
    y, n = ops.resample(torch.from_numpy(np.ascontiguousarray(x)).cuda(), O, M, lens=lens, skip=skip,
                        max_wav_value=mwv, pcm_scale=pcm, out=out)
    assert y is out and n.dtype == torch.int32 and n.shape == (B,)
    host = buf.cpu().numpy()
    R.check_guard(host, B, N_out)
    return R.split_guard(host, B, N_out)[0].copy(), n.cpu().numpy()


def _dev(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _check_rows(x, lens, O, M, N_out, y, n, mwv=32768.0, skip=None):
    h64 = R.table64(O, M)
    worst = 0.0
    for b, n_b in enumerate(lens):
        y64, S, m_b = R.model(R.as_read(x[b], mwv), n_b, 0 if skip is None else skip[b], O, M, N_out, h64)
        worst = max(worst, R.check(y[b], y64, S, m_b, h64.shape[1], name=f"({O}, {M}) row {b} of {n_b}"))
        assert n[b] == m_b, (b, n_b, int(n[b]), m_b)
    return worst


def test_tile_constant():
    import test_resample_cpu
    assert TILE == test_resample_cpu.TILE == 256


@pytest.mark.parametrize("kind, mwv", [("float32", None), ("int16", 32768.0)])
@pytest.mark.parametrize("O, M", R.RATIOS)
def test_matrix(O, M, kind, mwv):
    """Every row length of ``row_lengths`` in one ragged batch of capacity max + 5, poison behind the rows and in the
    output, lengths as a device tensor."""
    x, lens = R.noise_batch(R.row_lengths(O, M, TILE), kind, 100 * O + M)
    assert x.shape[1] == max(lens) + 5
    N_out = R.length(max(lens), O, M) + 3
    y, n = _run(x, O, M, lens=_dev(lens), N_out=N_out, mwv=mwv)
    worst = _check_rows(x, lens, O, M, N_out, y, n)
    print(f"({O}, {M}) {kind}: worst error / bound {worst:.3f}")


def test_matrix_48000_to_22050():
    """One row of 4801 int16 samples through the 297-tap table, with a skip."""
    O, M = BIG
    x, lens = R.noise_batch([4801], "int16", 7)
    N_out = R.length(4801, O, M)
    y, n = _run(x, 48000, 22050, lens=_dev(lens), skip=_dev([5]), N_out=N_out, mwv=32768.0)
    worst = _check_rows(x, lens, O, M, N_out, y, n, skip=[5])
    print(f"(320, 147): worst error / bound {worst:.3f}")


@pytest.mark.parametrize("O, M", R.RATIOS + (BIG,))
def test_impulses(O, M):
    """Rows that are zero except one 0.75: every output is float32(table[r][j]) * float32(0.75) bit for bit where the
    impulse is in reach and exactly 0 elsewhere -- q, r, W and both ends of the tap range, with no tolerance."""
    from visual_onoma_to_wave_amd import ops
    x, n_b, ks = R.impulse_rows(O, M)
    N_out = R.length(n_b, O, M) + 3
    y, n = _run(x, O, M, lens=[n_b] * 3, N_out=N_out)
    h32 = ops.resample_table(O, M).numpy()
    assert h32.shape == (M, R.geometry(O, M)[3])
    for b, k in enumerate(ks):
        want = R.impulse_expected(h32, k, n_b, O, M, N_out)
        assert np.count_nonzero(want) > R.geometry(O, M)[2] * M // (2 * O)
        bad = np.flatnonzero(_bits(y[b]) != _bits(want))
        assert bad.size == 0, (O, M, k, int(bad[0]), y[b][bad[0]], want[bad[0]])
        assert n[b] == R.length(n_b, O, M)


@pytest.mark.parametrize("O, M", R.RATIOS)
def test_invariance_bit_for_bit(O, M):
    lens = R.row_lengths(O, M, TILE)
    x, _ = R.noise_batch(lens, "float32", 100 * O + M)
    N_out = R.length(max(lens), O, M) + 3
    y, n = _run(x, O, M, lens=lens, N_out=N_out)
    # a row of the ragged batch is the single-row call on its own samples
    for b, n_b in enumerate(lens):
        if n_b:
            y1, n1 = _run(x[b:b + 1, :n_b], O, M, N_out=N_out)
            assert _same(y1[0], y[b]) and n1[0] == n[b], (b, n_b)
    # skip = s is the skip = 0 result shifted by s; past the row's length it is clamped: nothing left
    b = 9
    L = R.length(lens[b], O, M)
    assert L >= 2 * TILE + 1 and n[b] == L
    for s in (1, TILE - 1, TILE, L - 1, L, L + 3):
        for sk in ([s], _dev([s])):
            ys, ns = _run(x[b:b + 1], O, M, lens=[lens[b]], skip=sk, N_out=N_out)
            m = max(L - s, 0)
            assert ns[0] == m, (s, int(ns[0]))
            assert _same(ys[0, :m], y[b, s:s + m]) and not ys[0, m:].any(), s
    # a smaller capacity is the prefix of the full result
    for cap in (7, TILE - 1, TILE, TILE + 1):
        yc, nc = _run(x, O, M, lens=lens, N_out=cap)
        assert _same(yc, y[:, :cap]) and np.array_equal(nc, np.minimum(n, cap)), cap


@pytest.mark.parametrize("mwv", [32768.0, 32767.0])
@pytest.mark.parametrize("O, M", [(3, 2), (2, 3)])
def test_int16_input_is_the_fp32_call_on_the_quotients(O, M, mwv):
    x16, lens = R.noise_batch(R.row_lengths(O, M, TILE), "int16", 100 * O + M)
    N_out = R.length(max(lens), O, M) + 3
    y16, n16 = _run(x16, O, M, lens=lens, N_out=N_out, mwv=mwv)
    yf, nf = _run(R.as_read(x16, mwv), O, M, lens=lens, N_out=N_out)
    assert _same(y16, yf) and np.array_equal(n16, nf)
    _check_rows(x16, lens, O, M, N_out, y16, n16, mwv=mwv)


@pytest.mark.parametrize("O, M", [(3, 2), (2, 3)])
def test_pcm_output(O, M):
    scale = 32768.0
    x, lens = R.noise_batch(R.row_lengths(O, M, TILE), "float32", 100 * O + M)
    N_out = R.length(max(lens), O, M) + 3
    y, n = _run(x, O, M, lens=lens, N_out=N_out)
    from visual_onoma_to_wave_amd import ops
    B = x.shape[0]
    buf = torch.from_numpy(PC.guarded(B, N_out)).cuda()
    q, nq = ops.resample(torch.from_numpy(x).cuda(), O, M, lens=lens, pcm_scale=scale,
                         out=buf[:B * N_out].view(B, N_out))
    assert np.array_equal(nq.cpu().numpy(), n)
    frac = PC.check_pcm(buf.cpu().numpy(), y, scale, rows=n.tolist(), name=f"({O}, {M})")
    print(f"({O}, {M}): band fraction {frac:.4f}")
    # a saturating row (steps between -1 and 1 overshoot) and a NaN sample: equality with the store's expression
    n_b = 900
    sat = np.where((np.arange(n_b) // 45) % 2 == 0, 1.0, -1.0).astype(np.float32)
    nan = np.random.default_rng(9).uniform(-0.5, 0.5, n_b).astype(np.float32)
    nan[n_b // 2] = np.nan
    xs = np.stack([sat, nan])
    ys, _ = _run(xs, O, M)
    qs, _ = _run(xs, O, M, pcm=scale)
    assert qs.dtype == np.int16 and np.array_equal(qs, PC.expected_pcm(ys, scale))
    assert (ys[0] > 1.0).any() and (ys[0] < -1.0).any() and qs[0].max() == 32767 and qs[0].min() == -32768
    assert np.isnan(ys[1]).any() and not np.isnan(ys[1]).all() and (qs[1][np.isnan(ys[1])] == 0).all()


def test_graph_replay_follows_its_inputs():
    from visual_onoma_to_wave_amd import ops
    O, M = 7, 5
    xa, la = R.noise_batch([700, 3, 512], "float32", 1)
    xb, lb = R.noise_batch([1, 705, 300], "float32", 2)
    xb = xb[:, :xa.shape[1]]
    N_out = R.length(xa.shape[1], O, M)
    x, lens, skip = torch.from_numpy(xa).cuda(), _dev(la), _dev([0, 1, 2])
    out = torch.full((3, N_out), float("nan"), device="cuda")
    ops.resample(x, O, M, lens=lens, skip=skip, out=out)  # warm: the table is built outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, n = ops.resample(x, O, M, lens=lens, skip=skip, out=out)
    for xs, ls, ss in ((xa, la, [0, 1, 2]), (xb, lb, [1, 300, 0]), (xa, [1, 3, 300], [0, 0, 600])):
        x.copy_(torch.from_numpy(xs))
        lens.copy_(torch.tensor(ls, dtype=torch.int32))
        skip.copy_(torch.tensor(ss, dtype=torch.int32))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got, got_n = y.cpu().numpy().copy(), n.cpu().numpy().copy()
        want, want_n = _run(xs, O, M, lens=ls, skip=ss, N_out=N_out)
        assert _same(got, want) and np.array_equal(got_n, want_n), (ls, ss)
        _check_rows(xs, ls, O, M, N_out, got, got_n, skip=ss)


def test_refusals_launch_nothing():
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    O, M, B, N, N_out = 3, 2, 2, 300, 200
    x32 = torch.zeros((B, N), device="cuda")
    x16 = torch.zeros((B, N), dtype=torch.int16, device="cuda")
    table = ops.resample_table(O, M, "cuda:0")
    y32 = torch.from_numpy(R.guarded(B, N_out, np.float32)).cuda()
    y16 = torch.from_numpy(R.guarded(B, N_out, np.int16)).cuda()
    ol = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    base = dict(x=x32, x16=0, mwv=32768.0, B=B, N=N, table=table, O=O, M=M, y=y32, y16=0, scale=0.0, N_out=N_out)
    nan, inf = float("nan"), float("inf")
    cases = [dict(x=None), dict(y=None), dict(table=None), dict(B=0), dict(B=65536), dict(N=0), dict(N_out=0),
             dict(O=4, M=2), dict(O=9, M=1), dict(O=1, M=1), dict(O=1025, M=1024), dict(O=0, M=1)]
    cases += [dict(x=x16, x16=1, mwv=v) for v in (0.0, -1.0, nan, inf)]
    cases += [dict(y=y16, y16=1, scale=v) for v in (0.0, -32768.0, nan, inf)]
    for c in cases:
        a = dict(base, **c)
        rc = L.vo_resample(p(a["x"]), a["x16"], a["mwv"], a["B"], a["N"], None, None, p(a["table"]), a["O"], a["M"],
                           p(a["y"]), a["y16"], a["scale"], a["N_out"], p(ol), None)
        assert rc == -1, (c, rc)
        assert L.vo_last_error().decode().startswith("resample:"), (c, L.vo_last_error())
    torch.cuda.synchronize()
    assert R.untouched(y32.cpu().numpy()) and R.untouched(y16.cpu().numpy()) and (ol.cpu() == -7).all()
    # the accepted call, for contrast, writes all of it
    assert L.vo_resample(p(x32), 0, 0.0, B, N, None, None, p(table), O, M, p(y32), 0, 0.0, N_out, p(ol), None) == 0
    torch.cuda.synchronize()
    assert not y32[:B * N_out].cpu().numpy().any() and ol.cpu().tolist() == [N_out, N_out]
    R.check_guard(y32.cpu().numpy(), B, N_out)

    with pytest.raises(ValueError, match="equal"):
        ops.resample(x32, 22050, 22050)
    with pytest.raises(ValueError, match="44101 / 22050"):
        ops.resample(x32, 44101, 22050)
    with pytest.raises(ValueError, match=r"lens must be 2 sample counts in \[0, 300\]"):
        ops.resample(x32, O, M, lens=[1, 2, 3])
    with pytest.raises(ValueError, match=r"lens must be 2 sample counts in \[0, 300\]"):
        ops.resample(x32, O, M, lens=[1, 301])
    with pytest.raises(ValueError, match="skip must be 2 sample counts"):
        ops.resample(x32, O, M, skip=[0, -1])
    with pytest.raises(ValueError, match="shape \\(2,\\)"):
        ops.resample(x32, O, M, lens=_dev([1, 2, 3]))
    with pytest.raises(ValueError, match="out must be"):
        ops.resample(x32, O, M, pcm_scale=32768.0, out=torch.empty((B, N_out), device="cuda"))
    with pytest.raises(ValueError, match="max_wav_value"):
        ops.resample(x32, O, M, max_wav_value=32768.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resample(x32.cpu(), O, M)


def test_audio_resample():
    from visual_onoma_to_wave_amd import audio, ops
    x, lens = R.noise_batch([500, 777], "float32", 3)
    xd = torch.from_numpy(x).cuda()
    rs = audio.Resample(48000, 22050)
    y, n = rs(xd, lengths=lens, skip=[0, 4])
    want, want_n = ops.resample(xd, 48000, 22050, lens=lens, skip=[0, 4])
    assert torch.equal(y, want) and torch.equal(n, want_n)
    assert y.shape == (2, audio.resample_length(x.shape[1], 48000, 22050))
    y1, n1 = rs(xd[0, :500].contiguous())
    assert y1.dim() == 1 and n1.dim() == 0 and int(n1) == audio.resample_length(500, 48000, 22050)
    assert torch.equal(y1[:int(n1)], want[0, :int(n1)])
    same = audio.Resample(22050, 22050)
    assert same(xd, lens)[0] is xd and same(xd, lens)[1] is lens


# ---------------------------------------------------------------------------------- callers

def _utterances(rates, seed=11):
    """One decaying tone with a little noise per rate, about 0.4 s each, and six character durations that fit the
    mel of the resampled, trimmed signal."""
    rng = np.random.default_rng(seed)
    wavs = []
    for i, sr in enumerate(rates):
        n = int(sr * (0.35 + 0.05 * i)) + 17 * i
        t = np.arange(n) / sr
        wavs.append((0.4 * np.sin(2 * np.pi * rng.uniform(100, 900) * t) * np.exp(-t)
                     + 0.02 * rng.standard_normal(n)).astype(np.float32))
    return wavs


def _durations(n_samples, rng):
    F = 1 + n_samples // 256
    d = rng.integers(1, 12, 6)
    return (d * min(1.0, (F - 1) / d.sum())).astype(int)


def _assert_features_equal(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        for k in ("mel", "energy", "kurtosis"):
            assert u[k].dtype == v[k].dtype and u[k].shape == v[k].shape, k
            assert np.array_equal(u[k], v[k], equal_nan=True), k


def test_feature_extractor_resamples_on_the_device():
    from helpers import configs
    from visual_onoma_to_wave_amd import audio, ops
    from visual_onoma_to_wave_amd.preprocessor import FeatureExtractor
    fx = FeatureExtractor(configs()[0])
    assert fx.sr == 22050
    rng = np.random.default_rng(5)
    wavs = _utterances([48000, 48000, 48000])
    starts = [0.0, 0.01, 0.05]
    skips = [int(22050 * s) for s in starts]
    n_res = [audio.resample_length(len(w), 48000, 22050) - k for w, k in zip(wavs, skips)]
    durs = [_durations(n, rng) for n in n_res]
    out = fx.process(wavs, durs, sr=48000, start=starts, return_wavs=True)
    res = [o["wav"] for o in out]
    assert [len(r) for r in res] == n_res and all(r.dtype == np.float32 for r in res)
    _assert_features_equal(out, fx.process(res, durs))
    for w, k, r in zip(wavs, skips, res):
        y, n = ops.resample(torch.from_numpy(w)[None].cuda(), 48000, 22050, skip=[k])
        assert int(n[0]) == len(r) and _same(y[0, :len(r)].cpu().numpy(), r)
    # at the config's rate nothing changes
    at = [r[:5000] for r in res]
    d22 = [_durations(5000, rng) for _ in at]
    _assert_features_equal(fx.process(at, d22, sr=22050), fx.process(at, d22))
    # mixed rates in one call are three separate calls
    rates = [48000, 22050, 16000]
    mixed = _utterances(rates, seed=12)
    n_mix = [audio.resample_length(len(w), r, 22050) for w, r in zip(mixed, rates)]
    dm = [_durations(n, rng) for n in n_mix]
    together = fx.process(mixed, dm, sr=rates, return_wavs=True)
    apart = [fx.process([w], [d], sr=r, return_wavs=True)[0] for w, d, r in zip(mixed, dm, rates)]
    _assert_features_equal(together, apart)
    assert all(_same(u["wav"], v["wav"]) for u, v in zip(together, apart))
    assert _same(together[1]["wav"], mixed[1])
    # the duration check uses the resampled length: these durations fit 48000 samples, not what is left of them
    long = [np.array([1 + len(wavs[0]) // 256])]
    assert long[0][0] > 1 + n_res[0] // 256
    with pytest.raises(ValueError, match=f"its {n_res[0]} samples give"):
        fx.process(wavs[:1], long, sr=48000)
    fx.process(wavs[:1], long)  # taken as 22050 Hz samples, they fit
    with pytest.raises(ValueError, match="44101 / 22050"):
        fx.process(wavs[:1], durs[:1], sr=44101)


def test_attach_waves_resamples_on_the_device(device):
    import segment_check as SC
    from visual_onoma_to_wave_amd import hifigan, ops
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    hop, fps, n_mels = 8, 16, 5
    Fs = [10, 16, 40, 23]
    rng = np.random.default_rng(21)
    n48 = [int(np.ceil(F * hop * 320 / 147)) + 9 for F in Fs]
    wavs = [rng.integers(-16384, 16385, n).astype(np.int16) for n in n48]
    mels = [rng.standard_normal((F, n_mels)).astype(np.float32) for F in Fs]
    starts = [0.0, 0.0002, 0.0, 0.0001]
    skips = [int(22050 * s) for s in starts]
    assert any(skips)
    corpus = DeviceCorpus.from_arrays(SC.utterances(mels), 4, 1, device)
    corpus.attach_waves(wavs, hop, sr=48000, target_sr=22050, start=starts)
    res = []
    for w, k in zip(wavs, skips):
        y, n = ops.resample(torch.from_numpy(w)[None].cuda(), 48000, 22050, skip=[k])
        res.append(y[0, :int(n[0])].cpu().numpy())
    assert corpus.n_samples == [len(r) for r in res] and not corpus.waves.is_int16
    s = hifigan.SegmentSampler(corpus, fps * hop, hop, 6, seed=3, mel_pad=-11.5129)
    for _ in range(2):
        at = s.position()
        x, y = s.draw()
        plan = SC.model_plan(list(range(len(mels))), at, s.seed, 6, fps, Fs)
        want = SC.model_batch(mels, res, plan, fps, hop, -11.5129)
        assert np.array_equal(s.plan.cpu().numpy(), plan)
        assert _same(y.cpu().numpy(), want["y"]) and _same(x.cpu().numpy(), want["x"])
    with pytest.raises(ValueError, match="the mel has 10"):
        corpus.attach_waves([w[:len(w) // 2] for w in wavs], hop, sr=48000, target_sr=22050)
    with pytest.raises(ValueError, match="sr needs target_sr"):
        corpus.attach_waves(wavs, hop, sr=48000)


def test_graphed_synthesis_delivers_at_another_rate(device):
    """``GraphedSynthesis(out_rate=48000, pcm_scale=32768.0)`` against ``ops.resample`` of what the object without
    either option returns, on the requests, the model and the bucket of tests/test_gpu_graphed_synthesis.py."""
    import graphed_case as G
    from helpers import configs, hifigan_arrays, hifigan_h, vtts_arrays
    from weights import load_into
    from visual_onoma_to_wave_amd import hifigan, ops
    from visual_onoma_to_wave_amd.model import vTTS
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    m = m.to(device).eval()
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.linear_layer.bias += G.DUR_BIAS_SHIFT
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    g = g.to(device)
    m.set_precision("mixed")
    g.set_compute_dtype(torch.bfloat16)
    plain = GraphedSynthesis(m, g, G.BATCH, G.MAX_SRC, G.CAP)
    gs = GraphedSynthesis(m, g, G.BATCH, G.MAX_SRC, G.CAP, pcm_scale=G.PCM_SCALE, out_rate=48000)
    cap = ops.resample_len(G.CAP * G.HOP, 147, 320)
    seen = set()
    for i in (0, 1):
        r = G.request_set(i)
        q = {k: None if v is None else torch.from_numpy(np.asarray(v)).cuda() for k, v in r.items()}
        ref = plain(**q)
        want, want_n = ops.resample(ref.wav, 22050, 48000, lens=ref.samples, pcm_scale=G.PCM_SCALE)
        res = gs(**q)
        torch.cuda.synchronize()
        assert res.wav.dtype == torch.int16 and res.wav.shape == (G.BATCH, cap)
        assert torch.equal(res.wav, want), f"set {i}: wav differs"
        assert res.samples.dtype == torch.int64 and torch.equal(res.samples, want_n.to(torch.int64)), i
        assert torch.equal(res.mel_len, ref.mel_len)
        assert res.samples.tolist() == [ops.resample_len(s, 147, 320) for s in ref.samples.tolist()]
        assert res.wav.any()
        seen.update(res.mel_len.tolist())
    assert gs.captures == 1 and plain.captures == 1 and len(seen) > 2
    with pytest.raises(ValueError, match="441 / 40"):
        GraphedSynthesis(m, g, G.BATCH, G.MAX_SRC, G.CAP, out_rate=2000)
