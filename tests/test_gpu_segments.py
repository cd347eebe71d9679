"""The vocoder's training batches on the GPU (vo_segment_batch, vo_segment_plan, hifigan.data.SegmentSampler,
HifiGanTrainer.step_graphed(sampler=...)).  Every output is a copy or one IEEE division and the
draw is integer arithmetic: every comparison is ``torch.equal``, the floats by their bits.  The numpy model is
tests/segment_check.py, which tests/test_segments_cpu.py holds against the published Philox known answers."""

import numpy as np
import pytest
import torch

import segment_check as C
from helpers import hifigan_arrays, hifigan_h
from weights import load_into

pytestmark = pytest.mark.gpu

FPS = 4
FS = [1, FPS - 1, FPS, FPS + 1, 3 * FPS + 2]
WG_SAMPLES = 2048  # the samples one workgroup of segment_batch_kernel writes (SEG_SAMPLES, csrc/segments.hip)
WG_FRAMES = 64     # and the frames (SEG_FRAMES)


def _sizes(hop):
    """F and N of the case matrix's fifteen utterances: every F with N = (F - 1) hop (one sample where that is none),
    F hop and F hop + hop - 1."""
    Fs = [F for F in FS for _ in range(3)]
    Ns = [max(n, 1) for F in FS for n in ((F - 1) * hop, F * hop, F * hop + hop - 1)]
    return Fs, Ns


def _corpus(mels, wavs, hop, device, max_wav_value=32768.0):
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    return DeviceCorpus.from_arrays(C.utterances(mels), 4, 1, device).attach_waves(wavs, hop, max_wav_value)


@pytest.fixture(scope="module")
def corpora(device):
    """(corpus, mels, wavs) of the case matrix by (hop, n_mels, kind, max_wav_value); packed once each."""
    made = {}

    def get(hop, n_mels, kind, mwv=32768.0):
        key = (hop, n_mels, kind, mwv)
        if key not in made:
            mels, wavs = C.make(*_sizes(hop), n_mels, kind, 16)
            made[key] = (_corpus(mels, wavs, hop, device, mwv), mels, wavs)
        return made[key]
    return get


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_equal(got, want, what=""):
    for k in ("y", "x", "frames", "status"):
        w = torch.from_numpy(want[k])
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k, got[k].dtype, tuple(got[k].shape))
        assert torch.equal(_bits(got[k].cpu()), _bits(w)), (what, k)


def _nan_out(B, fps, hop, n_mels, device):
    return {"y": torch.full((B, fps * hop), float("nan"), device=device),
            "x": torch.full((B, fps, n_mels), float("nan"), device=device),
            "frames": torch.full((B,), -7, dtype=torch.int32, device=device),
            "status": torch.full((B,), -7, dtype=torch.int32, device=device)}


def _matrix_rows():
    """start 0 and F - fps of every utterance, and every start of the three longest ones' first."""
    Fs, _ = _sizes(1)
    rows = []
    for u, F in enumerate(Fs):
        rows += [(u, 0)] + ([(u, F - FPS)] if F > FPS else [])
    rows += [(12, s) for s in range(1, 3 * FPS + 2 - FPS)]
    return rows


@pytest.mark.parametrize("hop", [256, 3])        # 16-byte sample vectors; sample by sample
@pytest.mark.parametrize("n_mels", [80, 5])      # 16-byte mel vectors; value by value
@pytest.mark.parametrize("kind, mwv", [("int16", 32768.0), ("int16", 32767.0), ("float32", 32768.0)])
def test_case_matrix(corpora, device, hop, n_mels, kind, mwv):
    from visual_onoma_to_wave_amd import ops
    corpus, mels, wavs = corpora(hop, n_mels, kind, mwv)
    if kind == "int16":
        assert all(w[0] == -32768 and w[-1] == 32767 for w in wavs if len(w) >= 2)
    else:
        assert max(float(np.abs(w).max()) for w in wavs) > 2.0
    rows = _matrix_rows()
    batches = [rows[i:i + 7] for i in range(0, len(rows) - 6, 7)] + [rows[-7:], [rows[-1]], [rows[0]]]  # B = 7 and 1
    assert {len(b) for b in batches} == {1, 7} and {r for b in batches for r in b} == set(rows)
    for mel_pad in (0.0, -11.5129):
        for plan in batches:
            out = _nan_out(len(plan), FPS, hop, n_mels, device)
            got = ops.segment_batch(corpus.struct, corpus.waves, torch.tensor(plan, dtype=torch.int32, device=device),
                                    FPS, hop, mel_pad, out=out)
            assert got is out
            want = C.model_batch(mels, wavs, plan, FPS, hop, mel_pad, mwv)
            assert not want["status"].any()
            _assert_equal(got, want, (plan, mel_pad))


@pytest.mark.parametrize("hop, fpss", [
    (1, (WG_SAMPLES - 1, WG_SAMPLES, WG_SAMPLES + 1)),            # fps hop one below, at and one above the count
    (8, (WG_SAMPLES // 8 - 1, WG_SAMPLES // 8, WG_SAMPLES // 8 + 1)),  # the vector path's nearest: eight below and above
    (3, (WG_SAMPLES // 3 + 1,)),                                  # 2049 samples at a hop that is not 1
])
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_workgroup_edges(device, hop, fpss, kind):
    """Rows of more than one workgroup in both tensors: fps hop around the 2048 samples of a workgroup, fps around
    multiples of its 64 frames (255 .. 257, 2047 .. 2049); utterances shorter than the segment, longer, and one that
    ends inside the last workgroup."""
    from visual_onoma_to_wave_amd import ops
    top = max(fpss)
    Fs = [5, top + 9, top - 1, 70]
    Ns = [F * hop + (hop - 1) * (i % 2) for i, F in enumerate(Fs)]
    mels, wavs = C.make(Fs, Ns, 8, kind, 17)
    corpus = _corpus(mels, wavs, hop, device)
    for fps in fpss:
        assert fps > WG_FRAMES
        plan = [(0, 0), (1, 0), (1, top + 9 - fps), (1, 5), (2, 0), (3, 0), (3, max(70 - fps, 0))]
        out = _nan_out(len(plan), fps, hop, 8, device)
        got = ops.segment_batch(corpus.struct, corpus.waves, torch.tensor(plan, dtype=torch.int32, device=device), fps,
                                hop, -11.5129, out=out)
        want = C.model_batch(mels, wavs, plan, fps, hop, -11.5129)
        assert not want["status"].any()
        _assert_equal(got, want, (fps, hop))


def test_misaligned_outputs_take_the_element_path(corpora, device):
    """hop 256 and 80 mels, but y and x four bytes past a 16-byte boundary: no vector is stored there."""
    from visual_onoma_to_wave_amd import ops
    corpus, mels, wavs = corpora(256, 80, "int16")
    plan = [(12, 3), (4, 0), (14, 10)]
    out = _nan_out(3, FPS, 256, 80, device)
    for k in ("y", "x"):
        out[k] = torch.full((out[k].numel() + 1,), float("nan"), device=device)[1:].view(out[k].shape)
        assert out[k].data_ptr() % 16 == 4
    got = ops.segment_batch(corpus.struct, corpus.waves, torch.tensor(plan, dtype=torch.int32, device=device), FPS,
                            256, 1.5, out=out)
    _assert_equal(got, C.model_batch(mels, wavs, plan, FPS, 256, 1.5))


@pytest.mark.parametrize("hop, n_mels, kind", [(256, 80, "int16"), (3, 5, "float32")])
def test_refused_rows(corpora, device, hop, n_mels, kind):
    from visual_onoma_to_wave_amd import _lib, ops
    corpus, mels, wavs = corpora(hop, n_mels, kind)
    U = len(mels)
    good = [(12, 3), (0, 0), (9, 1), (14, 10)]
    bad = [(-1, 0), (U, 0), (12, -1), (12, 3 * FPS + 2 - FPS + 1), (3, 1), (-2 ** 31, 0), (5, 2 ** 31 - 1)]
    plan = [bad[0], good[0], bad[1], bad[2], good[1], good[2], bad[3], bad[4], good[3], bad[5], bad[6]]
    mel_pad = -11.5129
    got = ops.segment_batch(corpus.struct, corpus.waves, torch.tensor(plan, dtype=torch.int32, device=device), FPS, hop,
                            mel_pad, out=_nan_out(len(plan), FPS, hop, n_mels, device))
    _assert_equal(got, C.model_batch(mels, wavs, plan, FPS, hop, mel_pad))
    is_bad = torch.tensor([r in bad for r in plan])
    assert got["status"].cpu().tolist() == [_lib.SEG_BAD_ROW if b else _lib.SEG_OK for b in is_bad.tolist()]
    assert not got["frames"].cpu()[is_bad].any() and not got["y"].cpu()[is_bad].any()
    assert torch.equal(got["x"].cpu()[is_bad], torch.full((len(bad), FPS, n_mels), mel_pad))
    alone = ops.segment_batch(corpus.struct, corpus.waves, torch.tensor(good, dtype=torch.int32, device=device), FPS,
                              hop, mel_pad)
    for k in ("y", "x", "frames", "status"):
        assert torch.equal(_bits(got[k][~is_bad.to(device)]), _bits(alone[k])), k


def test_argument_checks(corpora, device):
    from visual_onoma_to_wave_amd import ops
    corpus, mels, wavs = corpora(256, 80, "int16")
    other = _corpus(mels[:3], wavs[:3], 256, device)
    plan = torch.zeros((2, 2), dtype=torch.int32, device=device)
    sb = lambda p=plan, fps=FPS, hop=256, w=corpus.waves, **kw: ops.segment_batch(corpus.struct, w, p, fps, hop, **kw)  # noqa: E731
    for p in (plan.cpu(), plan.long(), plan.view(4), torch.zeros((2, 5), dtype=torch.int32, device=device)):
        with pytest.raises(ValueError, match=r"int32 \(B, 2\) tensor on the GPU"):
            sb(p)
    for kw, msg in (({"fps": 0}, "fps must be >= 1"), ({"hop": 0}, "hop must be >= 1"),
                    ({"fps": 2 ** 23, "hop": 256}, "at or above 2\\^31"), ({"w": other.waves}, "3 utterances")):
        with pytest.raises(ValueError, match=msg):
            sb(**kw)
    out = _nan_out(2, FPS, 256, 80, device)
    with pytest.raises(ValueError, match=r"out\['y'\]"):
        sb(out=dict(out, y=out["y"][:, :-1]))
    order, counter = torch.zeros(3, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int64, device=device)
    for o, c, seed, B, fps, msg in ((order.long(), counter, 0, 2, 4, "order must be"), (order[:0], counter, 0, 2, 4, "order must be"),
                                    (order, counter.int(), 0, 2, 4, "counter must be"), (order, counter, -1, 2, 4, "seed"),
                                    (order, counter, 0, 0, 4, "B must be"), (order, counter, 0, 65536, 4, "B must be"),
                                    (order, counter, 0, 2, 0, "fps must be")):
        with pytest.raises(ValueError, match=msg):
            ops.segment_plan(corpus.struct, o, c, seed, B, fps)
    assert counter.item() == 0  # nothing was launched


@pytest.mark.parametrize("start_at", [0, 2 ** 32 + 11])
def test_plan_kernel_matches_the_host_rule(corpora, device, start_at):
    """Three calls in a row advance the counter by B each; an ``order`` of five with an id outside the corpus, so a
    batch of seven wraps it; a counter pre-set above 2^32 reaches the second counter word of the generator."""
    from visual_onoma_to_wave_amd import ops
    from visual_onoma_to_wave_amd.hifigan import segment_plan_host
    corpus = corpora(256, 80, "int16")[0]
    B, seed = 7, 0x9E3779B97F4A7C15
    order = [12, 4, 15, 13, 0]  # 15 is outside [0, 15)
    order_d = torch.tensor(order, dtype=torch.int32, device=device)
    counter = torch.tensor([start_at], dtype=torch.int64, device=device)
    plan_d = torch.full((B, 2), -7, dtype=torch.int32, device=device)
    for call in range(3):
        assert counter.item() == start_at + call * B
        got = ops.segment_plan(corpus.struct, order_d, counter, seed, B, FPS, plan=plan_d)
        assert got is plan_d
        want = segment_plan_host(order, start_at + call * B, seed, B, FPS, corpus.n_frames)
        assert np.array_equal(got.cpu().numpy(), want), call
        assert np.array_equal(want, C.model_plan(order, start_at + call * B, seed, B, FPS, corpus.n_frames))
    assert counter.item() == start_at + 3 * B
    big = ops.segment_plan(corpus.struct, order_d, counter, seed, 300, FPS)  # more rows than the workgroup has lanes
    assert np.array_equal(big.cpu().numpy(), C.model_plan(order, start_at + 3 * B, seed, 300, FPS, corpus.n_frames))
    assert counter.item() == start_at + 3 * B + 300


def _model_draw(sampler, mels, wavs, counter, order=None):
    plan = C.model_plan(list(range(len(mels))) if order is None else order, counter, sampler.seed, sampler.batch,
                        sampler.fps, [m.shape[0] for m in mels])
    return plan, C.model_batch(mels, wavs, plan, sampler.fps, sampler.hop, sampler.mel_pad)


def test_graph_replay_of_the_draw(corpora, device):
    import visual_onoma_to_wave_amd  # noqa: F401  (before the first GPU call: its import-time runtime setting)
    from visual_onoma_to_wave_amd.hifigan import SegmentSampler
    corpus, mels, wavs = corpora(256, 80, "int16")
    s = SegmentSampler(corpus, FPS * 256, 256, 7, seed=99, mel_pad=-11.5129)
    assert s.epoch_steps == 3
    x, y = s.draw()  # warm outside the capture
    plan, want = _model_draw(s, mels, wavs, 0)
    assert np.array_equal(s.plan.cpu().numpy(), plan)
    _assert_equal({"y": y, "x": x, "frames": s.frames, "status": s.status}, want)
    assert s.position() == 7
    s.seek(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.draw(out=(x, y))
    assert s.position() == 0  # a capture runs nothing
    order = None
    for i, at in enumerate((0, 7, 14, 5000000000, 5000000007)):
        if i == 3:
            order = [int(v) for v in np.random.default_rng(3).permutation(len(mels))]
            s.set_order(order).seek(at)
        graph.replay()
        torch.cuda.synchronize()
        plan, want = _model_draw(s, mels, wavs, at, order)
        assert np.array_equal(s.plan.cpu().numpy(), plan), at
        _assert_equal({"y": y, "x": x, "frames": s.frames, "status": s.status}, want, at)
        assert s.position() == at + 7


def test_mel_from_the_drawn_audio(device):
    """``mel="audio"``: x is the HiFi-GAN training mel of the drawn y (fmax from h), whatever mel the corpus holds."""
    from visual_onoma_to_wave_amd import hifigan, ops
    h = hifigan.AttrDict(hifigan_h())
    hop, fps = h.hop_size, 8
    Fs = [5, 8, 11, 30]
    mels, wavs = C.make(Fs, [F * hop for F in Fs], 5, "float32", 18)
    wavs = [(w / 6).astype(np.float32) for w in wavs]
    corpus = _corpus(mels, wavs, hop, device)
    s = hifigan.SegmentSampler(corpus, fps * hop, hop, 3, seed=5, mel="audio", h=h)
    for out in (None, (torch.full((3, fps, h.num_mels), float("nan"), device=device),
                       torch.full((3, fps * hop), float("nan"), device=device))):
        at = s.position()
        x, y = s.draw(out=out)
        assert out is None or (x is out[0] and y is out[1])
        plan, want = _model_draw(s, mels, wavs, at)
        assert np.array_equal(s.plan.cpu().numpy(), plan)
        assert torch.equal(_bits(y.cpu()), _bits(torch.from_numpy(want["y"])))
        ref = ops.stft_mel_ex(y, s.window, s.fb, n_fft=h.n_fft, hop=hop, n_mels=h.num_mels, pad=(h.n_fft - hop) // 2,
                              mag_eps=1e-9)
        assert x.shape == (3, fps, h.num_mels) and torch.equal(x, ref.transpose(1, 2))
    with pytest.raises(ValueError, match="needs the vocoder's config"):
        hifigan.SegmentSampler(corpus, fps * hop, hop, 3, mel="audio")


def _gen(device):
    from visual_onoma_to_wave_amd import hifigan
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    return g.to(device)


def test_trainer_graphed_with_sampler_matches_eager(device):
    """``step_graphed(sampler=...)``, each replay a whole step with its batch, against eager ``sampler.draw`` +
    ``step`` from the same initial state and seed, at the shapes of test_trainer_graphed_matches_eager (B = 2, 32
    frames, segment 8192, fp32 compute, capturable AdamW): two epochs of four steps with an epoch boundary and a new
    order in between.  The drawn batches are equal (integer arithmetic) and every kernel of the step is
    deterministic, so parameters and losses must match bit for bit."""
    from visual_onoma_to_wave_amd import hifigan
    h = hifigan.AttrDict(hifigan_h())
    hop, seg, B = h.hop_size, 8192, 2
    Fs = [20, 32, 45, 33, 71]  # shorter than the segment, exactly it, longer
    mels, wavs = C.make(Fs, [F * hop for F in Fs], 80, "int16", 19)
    mels = [m - 4 for m in mels]
    wavs = [(w // 4).astype(np.int16) for w in wavs]
    corpus = _corpus(mels, wavs, hop, device)
    orders = [[0, 1, 2, 3, 4], [3, 0, 4, 2, 1]]
    finals = []
    for graphed in (False, True):
        torch.manual_seed(1234)
        g = _gen("cuda")
        tr = hifigan.HifiGanTrainer(g, h, graphed=graphed, capturable=True).set_compute_dtype(torch.float32)
        s = hifigan.SegmentSampler(corpus, seg, hop, B, seed=77, mel_pad=-11.5129)
        plans = []
        for epoch in range(2):
            s.set_order(orders[epoch])
            for _ in range(4):
                if graphed:
                    losses = tr.step_graphed(sampler=s, warmup=2)
                else:
                    x, y = s.draw()
                    losses = tr.step(x, y)
                plans.append(s.plan.cpu().numpy().copy())
            tr.end_epoch()
        torch.cuda.synchronize()
        for i, p in enumerate(plans):
            assert np.array_equal(p, C.model_plan(orders[i // 4], 2 * i, 77, B, seg // hop, Fs)), (graphed, i)
        assert s.position() == 16
        finals.append(({k: float(v) for k, v in losses.items()},
                       torch.cat([p.detach().flatten().cpu() for p in g.parameters()]),
                       torch.cat([p.detach().flatten().cpu() for p in tr.mpd.parameters()]),
                       torch.cat([p.detach().flatten().cpu() for p in tr.msd.parameters()])))
    (le, ge, pe, se), (lg, gg, pg, sg) = finals
    assert torch.equal(gg, ge) and torch.equal(pg, pe) and torch.equal(sg, se) and lg == le
    # tr is the graphed trainer: its batch cannot change after the capture
    x, y = s.draw()
    with pytest.raises(ValueError, match="not both"):
        tr.step_graphed(x, y, sampler=s)
    with pytest.raises(ValueError, match="captured with a sampler"):
        tr.step_graphed(x, y)
    with pytest.raises(ValueError, match="captured with a sampler"):
        tr.step_graphed(sampler=hifigan.SegmentSampler(corpus, seg, hop, B))
    with pytest.raises(ValueError, match="not both"):
        tr.step_graphed()
