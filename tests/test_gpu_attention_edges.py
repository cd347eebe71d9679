"""Every attention kernel (csrc/attention.hip, csrc/attention_bwd.hip) per element at its tile and length
edges against float64 (tests/attn_check.py: dtype-exact operands, derived element bars, guard bands around
every output and the workspace, inputs compared bit for bit).  A path is selected by dtype and knob alone:

  F1  attention_kernel<float>            B1   attn_bwd_dq_kernel<float> + attn_bwd_dkdv_kernel<float, 32>
  F2  attention_kernel<bf16> (att_cfg 1) B2   the bf16 version-1 pair, reached without lse
  F3  attention2_kernel                  B2L  the same pair, reached with lse under att_cfg 1
                                         B3   attn2_bwd_dq_kernel + attn2_bwd_dkdv_kernel<0>
                                         B3x  att_cfg 2: attn2_bwd_dkdv_kernel<2>

Each forward path runs with and without lse (bit-identical outputs).  A backward runs in isolation: o_in is
the float64 forward rounded to the dtype and lse the float64 lse rounded to fp32, so a forward defect can
neither hide nor cause a backward failure; one chained case per backward path feeds the GPU forward's own
out and lse (the production pairing of autograd.py).  PATHS / CASES are plain data (no GPU at import):
tests/test_attn_check.py runs the CPU emulation through every case and checks the coverage."""

import ctypes

import pytest
import torch

import attn_check as AC

pytestmark = pytest.mark.gpu

PATHS = {
    "F1": dict(kind="fwd", dt="f32", cfg=0),
    "F2": dict(kind="fwd", dt="bf16", cfg=1),
    "F3": dict(kind="fwd", dt="bf16", cfg=0),
    "B1": dict(kind="bwd", dt="f32", cfg=0, lse=False),
    "B2": dict(kind="bwd", dt="bf16", cfg=0, lse=False),
    "B2L": dict(kind="bwd", dt="bf16", cfg=1, lse=True),
    "B3": dict(kind="bwd", dt="bf16", cfg=0, lse=True),
    "B3x": dict(kind="bwd", dt="bf16", cfg=2, lse=True),
}

# (B, L, H, lens): the smallest shapes at which each edge exists
SHAPES = [
    (1, 1, 2, [1]),
    (3, 17, 2, [17, 1, 16]),
    (2, 63, 2, [63, 33]),
    (3, 64, 2, [64, 63, 1]),
    (3, 65, 2, [65, 64, 1]),        # the second key tile, query tile and workgroup hold one row
    (2, 97, 1, [97, 96]),           # one past three 32-query tiles (B1)
    (3, 129, 3, [129, 128, 65]),    # H = 3: 27 workgroups, 27 % 8 = 3 (xcd_grouped_id's remainder); odd tile count
    (2, 193, 2, [130, 193]),        # even tile count
    (2, 65, 2, None),
    (2, 1000, 2, [1000, 937]),      # the model's max_seq_len: 16 tiles, the last holds 40
]
DRAW_SHAPES = [SHAPES[4], SHAPES[6], SHAPES[7]]
LENS_OVER = [(2, 65, 2, [200, 66]), (2, 100, 2, [128, 101])]  # the result of lens = L
LENS_ZERO = (3, 65, 2, [0, 65, 40])
LENS_NEGATIVE = (2, 65, 2, [-3, 65])  # clamp(lens, 0, L): as lens = 0
CHAINED = SHAPES[6]
IDENTITY = [SHAPES[6], SHAPES[7]]

CASES = []  # (path, attn_check case)
for _p, _d in PATHS.items():
    for _s in SHAPES + LENS_OVER + [LENS_ZERO, LENS_NEGATIVE]:
        CASES.append((_p, AC.case(*_s, draw="flat", dt=_d["dt"], kind=_d["kind"])))
    for _draw in ("peaked", "ramp_up", "ramp_down", "poison_pad"):
        for _s in DRAW_SHAPES:
            CASES.append((_p, AC.case(*_s, draw=_draw, dt=_d["dt"], kind=_d["kind"])))
    CASES.append((_p, AC.case(*SHAPES[9], draw="peaked", dt=_d["dt"], kind=_d["kind"])))
    CASES.append((_p, AC.case(*LENS_OVER[0], draw="peaked", dt=_d["dt"], kind=_d["kind"])))
_IDS = [f"{p}-{c['name']}" for p, c in CASES]
assert len(set(_IDS)) == len(_IDS)

_REFS = {}  # shared, never modified: the float64 references per case name


def ref_fwd(c):
    key = AC.case(c["B"], c["L"], c["H"], c["lens"], draw=c["draw"], dt=c["dt"], kind="fwd")["name"]
    if key not in _REFS:
        _REFS[key] = AC.reference_fwd(c, AC.make(c))
    return _REFS[key]


def ref_bwd(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = AC.reference_bwd(c, AC.make(c), ref_fwd(c)["o_in"])
    return _REFS[c["name"]]


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Knobs:
    def __init__(self, cfg, xcd=0):
        self.cfg, self.xcd = cfg, xcd

    def __enter__(self):
        from visual_onoma_to_wave_amd import _lib
        _lib.lib().vo_tune(b"att_cfg", self.cfg)
        _lib.lib().vo_tune(b"att_xcd", self.xcd)

    def __exit__(self, *exc):
        from visual_onoma_to_wave_amd import _lib
        _lib.lib().vo_tune(b"att_cfg", 0)
        _lib.lib().vo_tune(b"att_xcd", 0)


def _dev(m, *names):
    return {n: (None if m[n] is None else m[n].cuda()) for n in names}


def _view(buf, like):
    return buf[AC.G:AC.G + like.numel()].view(like.shape)


def run_fwd(path, c, xcd=0):
    """vo_attention_lse into guarded out / lse, vo_attention into a second guarded out.  Returns m with the
    buffers read back."""
    from visual_onoma_to_wave_amd import _lib, ops
    L_ = _lib.lib()
    m = AC.make(c)
    d = _dev(m, "qkv", "lens", "out_buf", "lse_buf")
    out2 = m["out_buf"].cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (_vp(d["qkv"]), ops.vo_dtype(d["qkv"]), _vp(d["lens"]), c["B"], c["L"], c["H"], AC.DK, 1.0 / AC.DK ** 0.5)
    with _Knobs(PATHS[path]["cfg"], xcd):
        _lib.check(L_.vo_attention_lse(*args, _vp(_view(d["out_buf"], m["out"])),
                                       _vp(_view(d["lse_buf"], m["lse"])), st), "vo_attention_lse")
        _lib.check(L_.vo_attention(*args, _vp(_view(out2, m["out"])), st), "vo_attention")
        torch.cuda.synchronize()
    it = AC._INT[out2.dtype]
    assert torch.equal(out2.view(it), d["out_buf"].view(it)), f"{c['name']}: out differs with and without lse"
    m["out_buf"].copy_(d["out_buf"].cpu())
    m["lse_buf"].copy_(d["lse_buf"].cpu())
    m["after"] = dict(qkv=d["qkv"].cpu())
    return m


def run_bwd(path, c, xcd=0, chained=False):
    """vo_attention_bwd[_lse] with the test's own dqkv and workspace inside guard bands.  Returns (m, o_in)."""
    from visual_onoma_to_wave_amd import _lib, ops
    L_ = _lib.lib()
    p = PATHS[path]
    m = AC.make(c)
    B, L, H = c["B"], c["L"], c["H"]
    assert int(L_.vo_attention_bwd_workspace_size(B, L, H)) == 4 * m["ws"].numel()
    d = _dev(m, "qkv", "dout", "lens", "dqkv_buf", "ws_buf")
    with _Knobs(p["cfg"], xcd):
        if chained:
            o_in, lse = ops.attention(d["qkv"], d["lens"], H, with_lse=True)
        else:
            rf = ref_fwd(c)
            o_in, lse = rf["o_in"].cuda(), rf["lse_in"].cuda()
        o_keep = o_in.clone()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (_vp(d["qkv"]), _vp(o_in), _vp(d["dout"]), ops.vo_dtype(d["qkv"]), _vp(d["lens"]), B, L, H, AC.DK,
                1.0 / AC.DK ** 0.5)
        tail = (_vp(_view(d["dqkv_buf"], m["dqkv"])), _vp(_view(d["ws_buf"], m["ws"])), st)
        if p["lse"]:
            _lib.check(L_.vo_attention_bwd_lse(*head, _vp(lse), *tail), "vo_attention_bwd_lse")
        else:
            _lib.check(L_.vo_attention_bwd(*head, *tail), "vo_attention_bwd")
        torch.cuda.synchronize()
    it = AC._INT[o_in.dtype]
    assert torch.equal(o_in.view(it), o_keep.view(it)), f"{c['name']}: the input o_in changed"
    m["dqkv_buf"].copy_(d["dqkv_buf"].cpu())
    m["ws_buf"].copy_(d["ws_buf"].cpu())
    m["after"] = dict(qkv=d["qkv"].cpu(), dout=d["dout"].cpu())
    return m, o_in.cpu()


def _exact_zero_rows(c, m):
    """Utterances without a key: out and every gradient exactly 0, lse exactly +inf."""
    for b, n in enumerate(AC.key_counts(c)):
        if n == 0 and c["kind"] == "fwd":
            assert not bool(m["out"][b].float().abs().any()) and bool((m["lse"][b] == float("inf")).all()), c["name"]
        if n == 0 and c["kind"] == "bwd":
            assert not bool(m["dqkv"][b].float().abs().any()), c["name"]
    if c["kind"] == "bwd":  # masked keys: dK and dV exactly 0 (poison_pad: their K / V rows hold +-8192)
        D = c["H"] * AC.DK
        for b, n in enumerate(AC.key_counts(c)):
            assert not bool(m["dqkv"][b, n:, D:].float().abs().any()), (c["name"], b)


@pytest.mark.parametrize("path,c", CASES, ids=_IDS)
def test_attention_edge(path, c):
    if c["kind"] == "fwd":
        m = run_fwd(path, c)
        AC.verify(c, m, ref_fwd(c), after=m["after"])
    else:
        m, _ = run_bwd(path, c)
        AC.verify(c, m, ref_bwd(c), after=m["after"])
    _exact_zero_rows(c, m)


@pytest.mark.parametrize("path", [p for p, d in PATHS.items() if d["kind"] == "bwd"])
def test_attention_bwd_chained(path):
    """The production pairing: the backward consumes the GPU forward's own out and lse; the reference is
    the float64 backward at that out."""
    c = AC.case(*CHAINED, draw="flat", dt=PATHS[path]["dt"], kind="bwd")
    m, o_in = run_bwd(path, c, chained=True)
    AC.verify(c, m, AC.reference_bwd(c, m, o_in), after=m["after"])


def _outputs(path, c, xcd=0):
    if c["kind"] == "fwd":
        m = run_fwd(path, c, xcd)
        return [m["out"].view(AC._INT[m["out"].dtype]), m["lse"].view(torch.int32)]
    m, _ = run_bwd(path, c, xcd)
    return [m["dqkv"].view(AC._INT[m["dqkv"].dtype])]


@pytest.mark.parametrize("shape", IDENTITY, ids=["L129_H3", "L193_H2"])
@pytest.mark.parametrize("path", list(PATHS))
def test_attention_xcd_remap_is_bit_identical(path, shape):
    """att_xcd 1 (plain workgroup order) against att_xcd 0: the remap only relabels workgroups."""
    c = AC.case(*shape, draw="flat", dt=PATHS[path]["dt"], kind=PATHS[path]["kind"])
    for a, b in zip(_outputs(path, c, 0), _outputs(path, c, 1)):
        assert torch.equal(a, b), c["name"]


@pytest.mark.parametrize("shape", IDENTITY, ids=["L129_H3", "L193_H2"])
def test_attention_bwd_cfg2_is_bit_identical(shape):
    """attn2_bwd_dkdv_kernel<2> against <0>: the same operations in the same order."""
    c = AC.case(*shape, draw="flat", dt="bf16", kind="bwd")
    assert torch.equal(_outputs("B3", c)[0], _outputs("B3x", c)[0]), c["name"]
