"""Energy / duration controls as device tensors (vo_variance_head_ctl, ops.control_view): the heads bit for bit
against torch fp32 on the CPU, the whole model against the reference's goldens (tests/golden/make_goldens_ctrl.py)
and the oracle, a captured graph following controls changed in place, and the synthesis pipeline with keyword
controls.

The discontinuous steps (round, bucketize) are compared exactly, so every case keeps them away from their edges by
the fixture's own margins, asserted on the CPU before anything runs: exp(log_d) - 1 at least D_MARGIN from a
half-integer, the controlled energy at least E_MARGIN from the nearest bin edge (a device expf one ulp off, or a
last-ulp difference of a summation, cannot flip either).  Draws that miss move on to the next seed."""

import ctypes

import numpy as np
import pytest
import torch

import test_gpu_parity as P
from helpers import configs, golden, hifigan_arrays, hifigan_h, stats, vtts_arrays
from weights import load_into

pytestmark = pytest.mark.gpu

D_MARGIN, E_MARGIN = 5e-3, 5e-4
B, T, D = 3, 7, 256  # 21 rows: the last 4-row block is partial
LENS = [7, 5, 0]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
          (torch.float32, torch.bfloat16)]
VO_ERR_INVALID = -1
SENTINEL = -12345.0


# ------------------------------------------------------------------------------ shared CPU side

def d_margin(log_d, valid=None):
    r = np.exp(np.asarray(log_d, np.float64)) - 1.0
    m = np.abs(r - (np.floor(r) + 0.5))
    return float((m if valid is None else m[valid]).min())


def e_margin(e, bins, valid=None):
    m = np.abs(np.asarray(e, np.float64)[..., None] - np.asarray(bins, np.float64)).min(-1)
    return float((m if valid is None else m[valid]).min())


def energy_bins():
    e_min, e_max, mean, std = stats()["energy"]
    return torch.linspace(e_min, e_max, 255), float(mean), float(std)


def views(base):
    """The accepted control shapes, and two non-contiguous views, of one 42-float base (on its device)."""
    return {
        "0-d": base[4],
        "(1,)": base[5:6],
        "(T,)": base[3:3 + T],
        "(1,T)": base[:T].reshape(1, T),
        "(B,1)": base[8:8 + B].reshape(B, 1),
        "(B,T)": base[:B * T].reshape(B, T),
        "(T,B).T": base[:B * T].reshape(T, B).T,
        "(B,14)[:,::2]": base.reshape(B, 14)[:, ::2],
    }


VIEW_NAMES = list(views(torch.zeros(B * 14)))
SHAPE_NAMES = VIEW_NAMES[:6]


def pad_mask():
    return torch.arange(T)[None, :] >= torch.tensor(LENS)[:, None]


def head_inputs(vals, h_dtype):
    """h (B, T, D) with h[..., 0] = vals and a one-hot weight: the head's prediction equals vals exactly (every other
    product is x * 0, the wave sum adds zeros, the bias is 0).  vals are bf16 values, so both h dtypes hold them."""
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, T, D, generator=g)
    h[..., 0] = vals
    w = torch.zeros(D)
    w[0] = 1.0
    return h.to(h_dtype).cuda(), w.cuda(), torch.tensor(LENS, dtype=torch.int32).cuda()


def log_d_values():
    """exp(v) - 1 spread over 0.2 ... 9.3, each about a quarter away from a half-integer."""
    k = torch.arange(B * T, dtype=torch.float32)
    target = 0.2 + (k * 3 % 10) + 0.1 * (k % 2)
    v = torch.log1p(target).to(torch.bfloat16).float().reshape(B, T)
    assert d_margin(v.numpy()) >= D_MARGIN
    return v


def duration_ref(vals, c):
    """modules.py:110-113 in torch fp32 on the CPU, on the masked prediction."""
    pred = vals.masked_fill(pad_mask(), 0.0)
    return pred, torch.clamp(torch.round(torch.exp(pred) - 1) * c, min=0)


def d_control_base(seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B * 14, generator=g) * 2.5
    base[0], base[1], base[2] = 0.0, 1.0, -0.75  # exact 0 and 1, and a negative product for the clamp
    return base


def energy_ref(vals, c, bins, mean, std):
    """modules.py:58-62 in torch fp32 on the CPU, one rounded operation per step."""
    pred = vals.masked_fill(pad_mask(), 0.0)
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    v = pred * f(std) + f(mean)
    v = v * c
    v = (v - f(mean)) / f(std)
    return v, torch.bucketize(v, bins)


def energy_case(name):
    """(vals, control base) of the first seed whose controlled energies keep E_MARGIN from every bin edge under the
    view ``name``, pad rows included (they are computed and compared too)."""
    bins, mean, std = energy_bins()
    for seed in range(200):
        g = torch.Generator().manual_seed(1000 + seed)
        vals = (torch.rand(B, T, generator=g) * 4.5 - 1.0).to(torch.bfloat16).float()
        base = torch.rand(B * 14, generator=g) * 1.1 + 0.5
        v, _ = energy_ref(vals, torch.broadcast_to(views(base)[name], (B, T)), bins, mean, std)
        if e_margin(v.numpy(), bins.numpy()) >= E_MARGIN:
            return vals, base
    raise AssertionError("no draw met the energy margin")


def run_duration(h, w, lens, control):
    from visual_onoma_to_wave_amd import ops
    pred, dr = ops.duration_head(h, w, 0.0, lens, d_control=control)
    torch.cuda.synchronize()
    return pred.cpu(), dr.cpu()


def run_energy(h, w, lens, x, bins, table, control, target=None):
    from visual_onoma_to_wave_amd import ops
    x = x.clone()
    _, mean, std = energy_bins()
    pred, idx = ops.energy_head(h, w, 0.0, lens, x, bins, table, target=target, mean=mean, std=std, control=control,
                                want_index=True)
    torch.cuda.synchronize()
    return pred.cpu(), idx.cpu(), x.cpu()


def energy_operands(x_dtype):
    g = torch.Generator().manual_seed(5)
    table = torch.randn(256, D, generator=g)
    x = torch.randn(B, T, D, generator=g).to(x_dtype)
    return x, table


# ------------------------------------------------------------------------------ head level

@pytest.mark.parametrize("name", VIEW_NAMES)
def test_duration_head_tensor_control_exact(name):
    vals = log_d_values()
    base = d_control_base(11)
    c_cpu = torch.broadcast_to(views(base)[name], (B, T))
    want_pred, want_dr = duration_ref(vals, c_cpu)
    if name in ("(B,T)", "(T,B).T", "(B,14)[:,::2]"):
        assert (want_dr[~pad_mask()] == 0).any() and (c_cpu < 0).any()  # the clamp and a zero control are exercised
    ctl = views(base.cuda())[name]
    for h_dtype in (torch.float32, torch.bfloat16):
        pred, dr = run_duration(*head_inputs(vals, h_dtype), ctl)
        np.testing.assert_array_equal(pred.numpy(), want_pred.numpy())
        np.testing.assert_array_equal(dr.numpy(), want_dr.numpy(), err_msg=f"{name} {h_dtype}")


@pytest.mark.parametrize("name", VIEW_NAMES)
def test_energy_head_tensor_control_exact(name):
    bins, mean, std = energy_bins()
    vals, base = energy_case(name)
    want_pred, want_idx = energy_ref(vals, torch.broadcast_to(views(base)[name], (B, T)), bins, mean, std)
    assert len(set(want_idx.flatten().tolist())) > 10  # the controls spread the tokens over many bins
    ctl = views(base.cuda())[name]
    for h_dtype, x_dtype in DTYPES:
        x, table = energy_operands(x_dtype)
        want_x = (x.float() + table[want_idx]).to(x_dtype)
        pred, idx, xo = run_energy(*head_inputs(vals, h_dtype), x.cuda(), bins.cuda(), table.cuda(), ctl)
        tag = f"{name} h {h_dtype} x {x_dtype}"
        np.testing.assert_array_equal(pred.numpy(), want_pred.numpy(), err_msg=tag)
        np.testing.assert_array_equal(idx.numpy(), want_idx.numpy().astype(np.int32), err_msg=tag)
        assert torch.equal(xo, want_x), tag


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_constant_tensor_equals_float_path(name):
    """A control tensor filled with one constant gives the bits of the Python-number entry with that constant."""
    c = 1.3
    ctl = views(torch.full((B * 14,), c).cuda())[name]
    bins, _, _ = energy_bins()
    vals = log_d_values()
    for h_dtype, x_dtype in DTYPES:
        hwl = head_inputs(vals, h_dtype)
        a, b = run_duration(*hwl, ctl), run_duration(*hwl, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(b[1], run_duration(*hwl, 1.0)[1])  # and the constant matters
        x, table = energy_operands(x_dtype)
        ops_ = (x.cuda(), bins.cuda(), table.cuda())
        hwl = head_inputs(vals - 1.0, h_dtype)
        a, b = run_energy(*hwl, *ops_, ctl), run_energy(*hwl, *ops_, c)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert not torch.equal(b[1], run_energy(*hwl, *ops_, 1.0)[1])


def test_energy_target_ignores_tensor_control():
    bins, _, _ = energy_bins()
    vals, base = energy_case("(B,T)")
    g = torch.Generator().manual_seed(9)
    target = (torch.rand(B, T, generator=g) * 5 - 1).cuda()
    x, table = energy_operands(torch.float32)
    hwl, ops_ = head_inputs(vals, torch.float32), (x.cuda(), bins.cuda(), table.cuda())
    a = run_energy(*hwl, *ops_, views(base.cuda())["(B,T)"], target=target)
    b = run_energy(*hwl, *ops_, 1.0, target=target)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    np.testing.assert_array_equal(a[1].numpy(), torch.bucketize(target.cpu(), bins).numpy())


def _desc(kind, h, w, lens, pred, dr=None, x=None, bins=None, table=None):
    from visual_onoma_to_wave_amd import _lib, ops
    d = _lib.HeadDesc()
    d.kind = kind
    d.h, d.h_dtype = h.data_ptr(), ops.vo_dtype(h)
    d.w, d.b, d.lens = w.data_ptr(), 0.0, lens.data_ptr()
    d.B, d.T, d.D = B, T, D
    d.pred = pred.data_ptr()
    d.d_control = d.e_control = 1.0
    d.e_mean, d.e_std = 0.0, 1.0
    d.x_dtype = ops.vo_dtype(h)
    if dr is not None:
        d.d_round = dr.data_ptr()
    if x is not None:
        d.x, d.bins, d.n_bins, d.table = x.data_ptr(), bins.data_ptr(), bins.numel(), table.data_ptr()
    return d


@pytest.mark.parametrize("kind", ["duration", "energy"])
@pytest.mark.parametrize("case,word", [("null", "null control"), ("negative", "negative stride"),
                                       ("short", "reaches past"), ("short_b", "reaches past")])
def test_entry_refuses_and_launches_nothing(kind, case, word):
    """VO_ERR_INVALID with a message, and the outputs keep their sentinel: nothing was launched."""
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    h, w, lens = head_inputs(log_d_values(), torch.float32)
    pred = torch.full((B, T), SENTINEL, device="cuda")
    dr = torch.full((B, T), SENTINEL, device="cuda")
    x = torch.full((B, T, D), SENTINEL, device="cuda")
    bins, _, _ = energy_bins()
    bins, table = bins.cuda(), torch.ones(256, D, device="cuda")
    ctl = torch.ones(B, T, device="cuda")
    d = _desc(_lib.HEAD_DURATION, h, w, lens, pred, dr=dr) if kind == "duration" else \
        _desc(_lib.HEAD_ENERGY, h, w, lens, pred, x=x, bins=bins, table=table)
    args = {"null": (None, B * T, T, 1), "negative": (ctl.data_ptr(), B * T, T, -1),
            "short": (ctl.data_ptr(), B * T - 1, T, 1), "short_b": (ctl.data_ptr(), B - 1, 1, 0)}[case]
    rc = L.vo_variance_head_ctl(ctypes.byref(d), *args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = L.vo_last_error().decode()
    torch.cuda.synchronize()
    assert rc == VO_ERR_INVALID and word in msg, (rc, msg)
    for out in (pred, dr, x):
        assert bool((out == SENTINEL).all())
    # the same descriptor with the full extent is accepted
    rc = L.vo_variance_head_ctl(ctypes.byref(d), ctl.data_ptr(), B * T, T, 1,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and not bool((pred == SENTINEL).any())


def test_control_on_another_device_is_refused():
    from visual_onoma_to_wave_amd import ops
    ctl = torch.ones(B, T, device="cuda:0")
    with pytest.raises(ValueError, match="cuda:0.*cuda:1"):
        ops.control_view(ctl, B, T, device="cuda:1")  # a host-side comparison: cuda:1 need not exist
    if torch.cuda.device_count() > 1:
        h, w, lens = (a.to("cuda:1") for a in head_inputs(log_d_values(), torch.float32))
        with pytest.raises(ValueError, match="cuda:0.*cuda:1"):
            ops.duration_head(h, w, 0.0, lens, d_control=ctl)


def test_converted_controls_match_fp32():
    """fp64, integer and host controls are converted to fp32 on the activations' device."""
    vals = log_d_values()
    hwl = head_inputs(vals, torch.float32)
    base = d_control_base(11)
    want = run_duration(*hwl, views(base.cuda())["(B,T)"])
    for ctl in (views(base.double().cuda())["(B,T)"], views(base)["(B,T)"], views(base)["(B,T)"].numpy()):
        got = run_duration(*hwl, ctl)
        assert torch.equal(got[1], want[1])
    two = run_duration(*hwl, torch.full((T,), 2, dtype=torch.int64).cuda())
    assert torch.equal(two[1], run_duration(*hwl, 2.0)[1])


# ------------------------------------------------------------------------------ model level

@pytest.fixture(scope="module")
def vtts(device):
    from visual_onoma_to_wave_amd.model import vTTS
    m = vTTS(*configs())
    load_into(m, vtts_arrays())
    return m.to(device).eval()


class _bias_shift:
    """The goldens' duration-bias shift (make_goldens.DUR_BIAS_SHIFT); the bias gets its own bits back on exit."""

    def __init__(self, m, shift):
        self.b, self.shift = m.variance_adaptor.duration_predictor.linear_layer.bias, float(shift)

    def __enter__(self):
        with torch.no_grad():
            self.saved = self.b.detach().clone()
            self.b += self.shift

    def __exit__(self, *exc):
        with torch.no_grad():
            self.b.copy_(self.saved)


def _infer(m, g, **kw):
    args = (P.cuda(g["in_audiotypes"]), P.cuda(g["in_texts"]), P.cuda(g["in_src_lens"]), int(g["in_max_src_len"]),
            None, None, None, None, None, None, P.cuda(g["in_images"]), None, True)
    with torch.no_grad():
        return m(*args, **kw)


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
@pytest.mark.parametrize("tag", ["tok", "utt"])
def test_vtts_tensor_controls_vs_golden(vtts, tag, mode):
    P._prec(vtts, mode)
    g = golden("vtts_inf_ctrl_" + tag)
    assert float(g["d_margin"]) >= D_MARGIN and float(g["e_margin"]) >= E_MARGIN
    with _bias_shift(vtts, g["dur_bias_shift"]):
        out = _infer(vtts, g, e_control=P.cuda(g["e_control"]), d_control=P.cuda(g["d_control"]))
    P._check(out, g, P.F32_MODEL if mode == "fp32" else P.BF16)


def test_vtts_ones_tensor_gives_uncontrolled_lengths(vtts):
    P._prec(vtts, "fp32")
    g = golden("vtts_inf")
    with _bias_shift(vtts, g["dur_bias_shift"]):
        out = _infer(vtts, g, d_control=torch.ones(2, 5, device="cuda"), e_control=torch.ones((), device="cuda"))
    np.testing.assert_array_equal(out[9].cpu().numpy(), g["mel_lens_out"])
    P._check(out, g, P.F32_MODEL)


ORACLE_BATCH_SEED, ORACLE_CTRL_SEED = 300, 0  # src_lens [7, 6, 6]; margins 2.8e-2 and 1.4e-3 on the oracle's values


def _oracle_case():
    from visual_onoma_to_wave_amd import synth
    b = synth.acoustic_batch(ORACLE_BATCH_SEED, 3, 7, 20, ragged=True)
    rng = np.random.default_rng(ORACLE_CTRL_SEED)
    ec = rng.uniform(0.5, 1.6, size=(3, 7)).astype(np.float32)
    dc = rng.uniform(0.0, 2.5, size=(3, 7)).astype(np.float32)
    return b, ec, dc


@pytest.fixture(scope="module")
def oracle_run():
    """The oracle's 10-tuple on a B = 3, T_src = 7 batch with per-token controls (computed once)."""
    from oracle import acoustic as A
    b, ec, dc = _oracle_case()
    sd = A.complete_state_dict(vtts_arrays(), stats()["energy"])
    key = "variance_adaptor.duration_predictor.linear_layer.bias"
    sd[key] = sd[key] + 1.6
    t = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    with torch.no_grad():
        ref = A.vtts_forward(sd, t(b["audiotypes"]), t(b["texts"]), t(b["src_lens"]), int(b["max_src_len"]),
                             images=t(b["images"]), energy_stats=stats()["energy"], e_control=t(ec), d_control=t(dc))
    valid = ~ref[6].numpy()
    bins = sd["variance_adaptor.energy_bins"].numpy()
    assert d_margin(ref[4].numpy(), valid) >= D_MARGIN and e_margin(ref[2].numpy(), bins, valid) >= E_MARGIN
    return b, ec, dc, {n: o.numpy() for n, o in zip(P.NAMES, ref) if o is not None}


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_vtts_tensor_controls_vs_oracle(vtts, oracle_run, mode):
    b, ec, dc, ref = oracle_run
    P._prec(vtts, mode)
    g = {"in_" + k: np.asarray(v) for k, v in b.items()}
    with _bias_shift(vtts, 1.6):
        out = _infer(vtts, g, e_control=P.cuda(ec), d_control=P.cuda(dc))
    assert ref["mel_lens_out"].min() > 0 and len(set(ref["d_rounded"].flatten().tolist())) > 8
    P._check(out, ref, P.F32_MODEL if mode == "fp32" else P.BF16)


# ------------------------------------------------------------------------------ graph replay

def test_graph_replay_follows_controls_changed_in_place():
    from visual_onoma_to_wave_amd import ops
    bins, mean, std = energy_bins()
    vals_e, base_e = energy_case("(B,T)")
    h_d, w, lens = head_inputs(log_d_values(), torch.float32)
    h_e, _, _ = head_inputs(vals_e, torch.float32)
    x0, table = energy_operands(torch.float32)
    x0, table, bins = x0.cuda(), table.cuda(), bins.cuda()
    dc = views(d_control_base(11).cuda())["(B,T)"].clone()
    ec = views(base_e.cuda())["(B,T)"].clone()

    def step():
        x = x0.clone()
        log_d, dr = ops.duration_head(h_d, w, 0.0, lens, d_control=dc)
        e, idx = ops.energy_head(h_e, w, 0.0, lens, x, bins, table, mean=mean, std=std, control=ec, want_index=True)
        return log_d, dr, e, idx, x

    first = [o.clone() for o in step()]  # warm-up, and the captured controls' result
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(gout, first))
    dc.copy_(views(d_control_base(12).cuda())["(B,T)"])
    ec.copy_(torch.rand(B, T, generator=torch.Generator().manual_seed(2)) * 1.1 + 0.5)  # GPU against GPU: no margin
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in gout]
    want = step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    for i in (1, 2, 3, 4):  # d_round, e_pred, idx and x all moved with the controls
        assert not torch.equal(got[i], first[i])


# ------------------------------------------------------------------------------ pipeline

def test_pipeline_submit_takes_keyword_controls(vtts, device, oracle_run):
    """submit(..., e_control=ec, d_control=dc), the caller dropping both at once: the wav of the direct call."""
    from visual_onoma_to_wave_amd import hifigan
    from visual_onoma_to_wave_amd.pipeline import SynthesisPipeline
    b, ec, dc, _ = oracle_run
    gen = hifigan.Generator(hifigan.AttrDict(hifigan_h()))
    load_into(gen, hifigan_arrays())
    gen.eval()
    gen.remove_weight_norm()
    gen = gen.to(device)
    gen.set_compute_dtype(torch.bfloat16)
    P._prec(vtts, "mixed")
    args = (P.cuda(b["audiotypes"]), P.cuda(b["texts"]), P.cuda(b["src_lens"]), int(b["max_src_len"]),
            None, None, None, None, None, None, P.cuda(b["images"]), None, True)
    with _bias_shift(vtts, 1.6), torch.no_grad():
        out = vtts(*args, e_control=P.cuda(ec), d_control=P.cuda(dc))
        ref = gen.run(out[1]).cpu()
        pipe = SynthesisPipeline(vtts, gen)
        e_t, d_t = P.cuda(ec), P.cuda(dc)
        pipe.submit(*args, e_control=e_t, d_control=d_t)
        del e_t, d_t
        junk = [torch.full((3, 7), 1e4, device=device) for _ in range(4)]  # what their memory could be handed to
        got_out, wav = pipe.next_wav()
        torch.cuda.synchronize()
    assert len(junk) == 4 and pipe.pending() == 0
    assert torch.equal(got_out[5].cpu(), out[5].cpu()) and torch.equal(got_out[9].cpu(), out[9].cpu())
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(wav.cpu(), ref)
