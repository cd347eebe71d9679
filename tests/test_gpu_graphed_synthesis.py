"""pipeline.GraphedSynthesis: one graph replay from glyph strips to (int16) samples, and the
pieces it is built from: ``vocoder_infer(device_pcm=True)`` and ``GlyphBatch.to(device, n_chars)``.

The eager path every replay is compared with, bit for bit: free-running ``model(..., max_mel_len=CAP)`` followed by
``vocoder.run(out[1], out[9], pcm_scale)``.  Model and vocoder are those of tests/test_gpu_ragged_generator.py
(synthetic weights, mixed precision, bf16 vocoder) with the duration predictor's output bias shifted by +1.6, so
that the predicted lengths are not zero."""

import numpy as np
import pytest
import torch

import graphed_case as G
import pcm_check as PC
from helpers import configs, hifigan_arrays, hifigan_h
from helpers import vtts_arrays
from weights import load_into

pytestmark = pytest.mark.gpu

BATCH, MAX_SRC, CAP, HOP, SCALE = G.BATCH, G.MAX_SRC, G.CAP, G.HOP, G.PCM_SCALE


class _bias_shift:
    """The goldens' duration-bias shift (tests/test_gpu_ctrl.py); the bias gets its own bits back on exit."""

    def __init__(self, m, shift):
        self.b, self.shift = m.variance_adaptor.duration_predictor.linear_layer.bias, float(shift)

    def __enter__(self):
        with torch.no_grad():
            self.saved = self.b.detach().clone()
            self.b += self.shift

    def __exit__(self, *exc):
        with torch.no_grad():
            self.b.copy_(self.saved)


@pytest.fixture(scope="module")
def vtts(device):
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    m = m.to(device).eval()
    with _bias_shift(m, G.DUR_BIAS_SHIFT):
        yield m


@pytest.fixture(scope="module")
def gen(device):
    from visual_onoma_to_wave_amd import hifigan
    g = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(g, hifigan_arrays())
    g.eval()
    g.remove_weight_norm()
    return g.to(device)


def _mode(vtts, gen, mode):
    vtts.set_precision(mode)
    gen.set_compute_dtype(torch.float32 if mode == "fp32" else torch.bfloat16)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _request(i, n=BATCH):
    """Request set i on the device, cut to its first n requests: (positional args of a call, controls)."""
    r = G.request_set(i)
    ec, dc = r["e_control"], r["d_control"]
    if n < BATCH:  # the per-request part of a control
        ec = ec[:n] if ec is not None and ec.ndim == 2 else ec
        dc = dc[:n] if dc is not None and dc.ndim == 2 else dc
    return dict(audiotypes=_cuda(r["audiotypes"][:n]), src_lens=_cuda(r["src_lens"][:n]),
                images=_cuda(r["images"][:n]), texts=_cuda(r["texts"][:n]), e_control=_cuda(ec), d_control=_cuda(dc))


def _eager(vtts, gen, q, pcm, cap=CAP):
    """Path A on a full batch of device tensors ``q`` (the keys of ``_request``)."""
    with torch.no_grad():
        out = vtts(q["audiotypes"], q["texts"], q["src_lens"], MAX_SRC, None, None, cap, None, None, None, q["images"],
                   None, True, e_control=1.0 if q["e_control"] is None else q["e_control"],
                   d_control=1.0 if q["d_control"] is None else q["d_control"])
        return out, gen.run(out[1], out[9], pcm)


def _assert_equal(res, out, wav, n=BATCH, what=""):
    torch.cuda.synchronize()
    assert res.wav.dtype == wav.dtype and res.wav.shape == (n, CAP * HOP), (what, res.wav.dtype, res.wav.shape)
    assert torch.equal(res.wav, wav[:n]), f"{what}: wav differs from the eager call"
    mel_len = out[9][:n]
    assert res.mel_len.dtype == torch.int64 and torch.equal(res.mel_len, mel_len), what
    assert res.samples.dtype == torch.int64 and torch.equal(res.samples, torch.clamp(mel_len, max=CAP) * HOP), what
    assert res.truncated.dtype == torch.bool and torch.equal(res.truncated, mel_len > CAP), what
    assert len(res.outputs) == len(out) == 10
    for k, (a, b) in enumerate(zip(res.outputs, out)):
        if b is None:
            assert a is None, (what, k)
        else:
            assert a.dtype == b.dtype and torch.equal(a, b[:n]), f"{what}: model output {k} differs"
    for b, s in enumerate(res.samples.tolist()):
        assert not res.wav[b, s:].any(), f"{what}: utterance {b} is not 0 past its {s} samples"
    host = res.wavs()
    assert [len(w) for w in host] == res.samples.tolist()
    for b, w in enumerate(host):
        np.testing.assert_array_equal(w, wav[b, :len(w)].cpu().numpy())


def _gs(vtts, gen, pcm=None, **kw):
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    return GraphedSynthesis(vtts, gen, BATCH, MAX_SRC, CAP, pcm_scale=pcm, **kw)


# ------------------------------------------------------------------------------ 1: replay == eager

@pytest.mark.parametrize("pcm", [None, SCALE], ids=["fp32", "pcm16"])
def test_replay_equals_eager_bit_for_bit(vtts, gen, pcm):
    _mode(vtts, gen, "mixed")
    gs = _gs(vtts, gen, pcm)
    lens_seen = set()
    for i in range(3):
        q = _request(i)
        res = gs(**q)
        out, wav = _eager(vtts, gen, q, pcm)
        _assert_equal(res, out, wav, what=f"set {i}")
        lens = out[9].tolist()
        print(f"set {i}: mel_len {lens}")
        lens_seen.update(lens)
        if i == 0:
            assert len(set(lens)) > 1 and 0 < min(lens) and max(lens) <= CAP, "set 0 must be ragged and fit"
        if pcm is not None:  # the int16 samples are the truncated fp32 samples of the same eager run
            f32 = _eager(vtts, gen, q, None)[1].cpu().numpy()
            rows = [min(int(v), CAP) * HOP for v in lens]
            frac = PC.check_pcm(wav.cpu().numpy(), f32, pcm, rows=rows, name=f"set {i}")
            print(f"set {i}: band fraction {frac:.4f}")
    assert gs.captures == 1 and len(lens_seen) > 3
    # host arrays go the same way as device tensors (copied before the replay)
    r = G.request_set(1)
    res = gs(r["audiotypes"], r["src_lens"], r["images"], texts=r["texts"], e_control=r["e_control"],
             d_control=r["d_control"])
    out, wav = _eager(vtts, gen, _request(1), pcm)
    _assert_equal(res, out, wav, what="host arrays")
    assert gs.captures == 1


# ------------------------------------------------------------------------------ 2: against the oracle

def test_fp32_pcm_against_the_oracle(vtts, gen):
    """Per utterance ||q / scale - r|| <= 1e-4 ||r|| + sqrt(N) / scale: 1e-4 is the fp32 generator bar
    (test_gpu_ragged_generator.py), sqrt(N) / scale the truncation (below one step per sample)."""
    _mode(vtts, gen, "fp32")
    try:
        mel_len, waves = G.oracle_set0()
        res = _gs(vtts, gen, SCALE)(**_request(0))
        torch.cuda.synchronize()
        assert res.mel_len.tolist() == mel_len.tolist() and not res.truncated.any()
        for b, (q, r) in enumerate(zip(res.wavs(), waves)):
            assert q.dtype == np.int16 and q.shape == r.shape == (int(mel_len[b]) * HOP,)
            err = np.linalg.norm(q.astype(np.float64) / SCALE - r.astype(np.float64))
            bar = 1e-4 * np.linalg.norm(r.astype(np.float64)) + np.sqrt(len(r)) / SCALE
            print(f"utterance {b} ({len(r)} samples): error {err:.3e}, bar {bar:.3e} (||r|| {np.linalg.norm(r):.2f})")
            assert err <= bar, (b, err, bar)
    finally:
        _mode(vtts, gen, "mixed")


# ------------------------------------------------------------------------------ 3: overflow

def test_overflow_is_cropped_and_flagged(vtts, gen):
    _mode(vtts, gen, "mixed")
    q = _request(2)
    q["d_control"] = torch.tensor([[6.0], [1.0], [1.0]], device="cuda")
    gs = _gs(vtts, gen, SCALE)
    res = gs(**q)
    out, wav = _eager(vtts, gen, q, SCALE)
    _assert_equal(res, out, wav, what="overflow")
    assert res.truncated.tolist() == [True, False, False], res.mel_len.tolist()
    assert res.mel_len[0].item() > CAP and res.samples[0].item() == CAP * HOP
    assert res.wav[0, -HOP:].any(), "the cropped utterance runs to the end of the buffer"


# ------------------------------------------------------------------------------ 4: partial batches

@pytest.mark.parametrize("n", [1, 2])
def test_partial_batches(vtts, gen, n):
    _mode(vtts, gen, "mixed")
    gs = _gs(vtts, gen, SCALE)
    gs(**_request(0))  # rows n ... must not keep the previous call's requests
    res = gs(**_request(1, n))
    full = _request(1)
    for k, v in full.items():  # the eager batch: requests 0 ... n - 1, then copies of request 0
        if v is not None and v.dim() >= 1 and v.shape[0] == BATCH and k != "d_control":
            full[k] = torch.cat([v[:n]] + [v[:1]] * (BATCH - n))
    out, wav = _eager(vtts, gen, full, SCALE)
    _assert_equal(res, out, wav, n=n, what=f"n = {n}")
    assert res.wav.shape[0] == n and torch.equal(gs.inputs.images[n:], gs.inputs.images[:1].expand(BATCH - n, -1, -1, -1))
    assert torch.equal(gs.inputs.texts[n:], gs.inputs.texts[:1].expand(BATCH - n, -1)) and gs.inputs.texts.any()
    q = _request(1, n)
    q["texts"] = None  # no texts: the static rows hold zeros, not the earlier call's; the result is the same
    _assert_equal(gs(**q), out, wav, n=n, what=f"n = {n}, texts=None")
    assert not gs.inputs.texts.any()


# ------------------------------------------------------------------------------ 5: weights changed

def test_recaptures_when_the_weights_change(vtts, gen):
    from visual_onoma_to_wave_amd import _base
    _mode(vtts, gen, "mixed")
    gen_sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    vtts_sd = {k: v.detach().clone() for k, v in vtts.state_dict().items()}
    try:
        gs = _gs(vtts, gen, SCALE)
        q = _request(0)
        before = gs(**q).wav.clone()
        assert gs.captures == 1
        gs(**_request(1))
        assert gs.captures == 1

        sd = {k: v.clone() for k, v in gen_sd.items()}
        sd["conv_post.bias"] += 0.05
        gen.load_state_dict(sd)
        res = gs(**q)
        out, wav = _eager(vtts, gen, q, SCALE)
        _assert_equal(res, out, wav, what="conv_post.bias")
        assert gs.captures == 2 and not torch.equal(res.wav, before)

        sd = {k: v.clone() for k, v in vtts_sd.items()}
        sd["mel_linear.bias"] += 0.25
        vtts.load_state_dict(sd)
        mel_before = res.outputs[1].clone()
        res = gs(**q)
        out, wav = _eager(vtts, gen, q, SCALE)
        _assert_equal(res, out, wav, what="mel_linear.bias")
        assert gs.captures == 3 and not torch.equal(res.outputs[1], mel_before)

        _mode(vtts, gen, "fp32")
        res = gs(**q)
        out, wav = _eager(vtts, gen, q, SCALE)
        _assert_equal(res, out, wav, what="set_precision")
        assert gs.captures == 4
        gs(**q)
        assert gs.captures == 4
        _base.invalidate_packs(gen)
        _assert_equal(gs(**q), out, wav, what="invalidate_packs")
        assert gs.captures == 5
    finally:
        gen.load_state_dict(gen_sd)
        vtts.load_state_dict(vtts_sd)
        _mode(vtts, gen, "mixed")


def test_recaptures_after_a_precision_round_trip(vtts, gen):
    """A module keeps one pack: fp32 and back with an eager run in between brings the pack key back to the captured
    one while every pack was dropped and rebuilt.  The capture holds the packs it reads and compares them by identity,
    so the next call captures again; without the eager run nothing was rebuilt and nothing is captured."""
    _mode(vtts, gen, "mixed")
    gs = _gs(vtts, gen, SCALE)
    q = _request(0)
    gs(**q)
    out, wav = _eager(vtts, gen, q, SCALE)
    _mode(vtts, gen, "fp32")
    _mode(vtts, gen, "mixed")
    _assert_equal(gs(**q), out, wav, what="round trip without a run")
    assert gs.captures == 1
    _mode(vtts, gen, "fp32")
    _eager(vtts, gen, _request(1), SCALE)  # rebuilds every pack in fp32: the bf16 ones are dropped
    _mode(vtts, gen, "mixed")
    res = gs(**q)
    assert gs.captures == 2
    _assert_equal(res, out, wav, what="round trip with an eager run")
    _assert_equal(gs(**q), *_eager(vtts, gen, q, SCALE), what="after the eager run in mixed")
    assert gs.captures == 2  # the eager run reused the packs the second capture holds


def test_recaptures_when_a_submodule_is_replaced(vtts, gen):
    import copy
    _mode(vtts, gen, "mixed")
    gs = _gs(vtts, gen, SCALE)
    q = _request(0)
    before = gs(**q).wav.clone()
    old = gen.resblocks[11]
    new = copy.deepcopy(old)
    with torch.no_grad():
        new.convs2[2].bias += 0.5
    try:
        gen.resblocks[11] = new
        res = gs(**q)
        out, wav = _eager(vtts, gen, q, SCALE)
        _assert_equal(res, out, wav, what="replaced ResBlock")
        assert gs.captures == 2 and not torch.equal(res.wav, before)
    finally:
        gen.resblocks[11] = old


# ------------------------------------------------------------------------------ 6: errors

def test_errors(vtts, gen):
    from visual_onoma_to_wave_amd.pipeline import GraphedSynthesis
    _mode(vtts, gen, "mixed")
    with pytest.raises(ValueError, match="max_seq_len"):
        GraphedSynthesis(vtts, gen, BATCH, MAX_SRC, 1001)
    gs = _gs(vtts, gen, SCALE)
    q = _request(0)
    vtts.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            gs(**q)
    finally:
        vtts.eval()
    gen.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            gs(**q)
    finally:
        gen.eval()
    four = {k: (torch.cat([v, v[:1]]) if v is not None else None) for k, v in q.items()}
    with pytest.raises(ValueError, match="batch = 3"):
        gs(**four)
    shape = tuple(gs.inputs.images.shape)
    assert shape == (BATCH, 1, 24, 102 * MAX_SRC)
    bad = dict(q, images=q["images"][..., :-102].contiguous())
    with pytest.raises(ValueError, match=r"\(3, 1, 24, 714\)"):
        gs(**bad)
    with pytest.raises(ValueError, match=r"\(2, 1, 24, 714\)"):
        gs(q["audiotypes"][:2], q["src_lens"][:2], q["images"])
    assert gs.captures == 0  # nothing ran


# ------------------------------------------------------------------------------ 7: no growth, no host wait

def test_no_allocation_growth_and_back_to_back_calls(vtts, gen):
    _mode(vtts, gen, "mixed")
    gs = _gs(vtts, gen, SCALE)
    qs = [_request(i) for i in range(3)]
    want = [_eager(vtts, gen, q, SCALE) for q in qs]
    gs(**qs[0])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for k in range(10):
        gs(**qs[k % 3])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    # two calls with no host wait in between: the first result, cloned in stream order, is still the first's
    first = gs(**qs[1]).wav.clone()
    second = gs(**qs[2])
    torch.cuda.synchronize()
    assert torch.equal(first, want[1][1])
    _assert_equal(second, *want[2], what="second of two calls")
    assert gs.captures == 1


# ------------------------------------------------------------------------------ 8: vocoder_infer

def test_vocoder_infer_device_pcm(gen):
    """The mels and sample counts of test_vocoder_infer_ragged_equals_per_utterance_calls: no |y * scale| reaches
    32768 there, so the device store and the host cast agree on every sample."""
    from visual_onoma_to_wave_amd.utils.model import vocoder_infer
    pre, model_cfg, _ = configs()
    gen.set_compute_dtype(torch.bfloat16)
    mel, lengths = G.infer_mels()
    samples = [40 * HOP, 23 * HOP - 100, 8 * HOP - 255, 300]
    mels = mel.transpose(1, 2).contiguous().cuda()
    scale = float(pre["audio"]["max_wav_value"])
    with torch.no_grad():
        y = gen(mels, lengths=[-(-n // HOP) for n in samples]).squeeze(1).cpu().numpy()
        yd = gen(mels).squeeze(1).cpu().numpy()
    assert np.abs(y * np.float32(scale)).max() < 32768 and np.abs(yd * np.float32(scale)).max() < 32768
    for kw in (dict(ragged=True), dict()):
        host = vocoder_infer(mels, gen, model_cfg, pre, lengths=samples, **kw)
        dev = vocoder_infer(mels, gen, model_cfg, pre, lengths=samples, device_pcm=True, **kw)
        assert [w.shape[0] for w in dev] == samples and all(w.dtype == np.int16 for w in dev)
        for a, b in zip(host, dev):
            np.testing.assert_array_equal(a, b)
    # without Normalize the keyword changes nothing: fp32 out
    raw = vocoder_infer(mels, gen, model_cfg, pre, lengths=samples, Normalize=False, device_pcm=True)
    assert all(w.dtype == np.float32 for w in raw)


# ------------------------------------------------------------------------------ 9: GlyphBatch.to

@pytest.mark.parametrize("stride", [1, 3])
def test_glyph_batch_at_bucket_width(device, stride):
    import torch.nn.functional as F
    from visual_onoma_to_wave_amd.dataset import GlyphBatch
    rng = np.random.default_rng(5)
    cell, H = 102, 24
    widths = [rng.integers(20, cell + 1, size=k) for k in (5, 2, 7)]
    strips = [rng.integers(0, 256, size=(H, int(w.sum()) + 3), dtype=np.uint8) for w in widths]
    batch = GlyphBatch(strips, widths, cell, stride)
    own = batch.to(device)
    assert own.shape == (3, 1, H, 7 * cell + 2 * (stride // 2) * cell)
    wide = batch.to(device, n_chars=9)
    assert wide.shape == (3, 1, H, 9 * cell + 2 * (stride // 2) * cell)
    assert torch.equal(wide, F.pad(own, (0, 2 * cell), value=1.0))
    assert torch.equal(batch.to(device, n_chars=7), own)
    with pytest.raises(ValueError, match="n_chars"):
        batch.to(device, n_chars=6)
