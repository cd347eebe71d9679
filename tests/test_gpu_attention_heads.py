"""The attention kernels at head sizes d_k = 64 and 32 (csrc/attention.hip, csrc/attention_bwd.hip: every kernel
is a template on DK) per element against float64 -- tests/test_gpu_attention_edges.py's matrix at the new
sizes, with its eight paths, tests/attn_check.py's derived bars and guard bands, and attn_check.DK set per case.

Head counts: d_k = 64 runs with H = 4 (odd case 5), d_k = 32 with H = 8 (odd case 7).  No head count appears
with two head sizes or in the d_k = 128 matrix, and the references are cached here by (d_k, case name), never
in test_gpu_attention_edges._REFS.  PATHS / CASES are plain data (no GPU at import): tests/test_heads_cpu.py
runs the CPU emulation through every case."""

import ctypes

import pytest
import torch

import attn_check as AC
import test_gpu_attention_edges as E

pytestmark = pytest.mark.gpu

PATHS = E.PATHS
HEADS = {64: (4, 5), 32: (8, 7)}  # d_k -> (H, the odd H of the xcd-remainder case)


def shapes(dk):
    """(B, L, H, lens): the smallest shapes at which each edge exists."""
    H, Ho = HEADS[dk]
    return [
        (1, 1, H, [1]),
        (3, 17, H, [17, 1, 16]),
        (3, 64, H, [64, 63, 1]),
        (3, 65, H, [65, 64, 1]),          # the second key tile, query tile and workgroup hold one row
        (2, 97, H, [97, 96]),             # one past three 32-query tiles (B1)
        (3, 129, Ho, [129, 128, 65]),     # 9 Ho = 45 / 63 workgroups: 5 / 7 mod 8 (xcd_grouped_id's remainder)
        (2, 193, H, [130, 193]),          # even tile count
        (2, 65, H, None),
    ]


def lens_over(dk):
    return (2, 65, HEADS[dk][0], [200, 66])  # the result of lens = L


def lens_zero(dk):
    return (3, 65, HEADS[dk][0], [0, 65, 40])


def lens_negative(dk):
    return (2, 65, HEADS[dk][0], [-3, 65])  # clamp(lens, 0, L): as lens = 0


def long_shape(dk):
    return (2, 1000, HEADS[dk][0], [1000, 937])  # the model's max_seq_len: 16 tiles, the last holds 40


def draw_shapes(dk):
    s = shapes(dk)
    return [s[3], s[5], s[6]]  # L = 65, 129, 193


def chained(dk):
    return shapes(dk)[5]


def identity(dk):
    return [shapes(dk)[5], shapes(dk)[6]]


CASES = []  # (d_k, path, attn_check case)
for _dk in HEADS:
    for _p, _d in PATHS.items():
        for _s in shapes(_dk) + [lens_over(_dk), lens_zero(_dk), lens_negative(_dk)]:
            CASES.append((_dk, _p, AC.case(*_s, draw="flat", dt=_d["dt"], kind=_d["kind"])))
        for _draw in ("peaked", "ramp_up", "ramp_down", "poison_pad"):
            for _s in draw_shapes(_dk):
                CASES.append((_dk, _p, AC.case(*_s, draw=_draw, dt=_d["dt"], kind=_d["kind"])))
        CASES.append((_dk, _p, AC.case(*long_shape(_dk), draw="peaked", dt=_d["dt"], kind=_d["kind"])))
_IDS = [f"dk{dk}-{p}-{c['name']}" for dk, p, c in CASES]
assert len(set(_IDS)) == len(_IDS)
assert not {c["H"] for _, _, c in CASES} & {c["H"] for _, c in E.CASES}  # no case name of the d_k = 128 matrix

_REFS = {}  # shared, never modified: the float64 references per (d_k, case name)


@pytest.fixture
def head_size(monkeypatch):
    """Sets attn_check.DK (read at call time by every function of attn_check and of the edges module)."""
    def set_dk(dk):
        monkeypatch.setattr(AC, "DK", dk)
    return set_dk


def ref_fwd(dk, c):
    assert AC.DK == dk
    key = (dk, AC.case(c["B"], c["L"], c["H"], c["lens"], draw=c["draw"], dt=c["dt"], kind="fwd")["name"])
    if key not in _REFS:
        _REFS[key] = AC.reference_fwd(c, AC.make(c))
    return _REFS[key]


def ref_bwd(dk, c):
    assert AC.DK == dk
    if (dk, c["name"]) not in _REFS:
        _REFS[dk, c["name"]] = AC.reference_bwd(c, AC.make(c), ref_fwd(dk, c)["o_in"])
    return _REFS[dk, c["name"]]


def run_bwd(dk, path, c, xcd=0, chained=False):
    """vo_attention_bwd[_lse] at d_k = dk with the test's own dqkv and workspace inside guard bands (the edges
    module's run_bwd with this module's reference cache).  Returns (m, o_in)."""
    from visual_onoma_to_wave_amd import _lib, ops
    L_ = _lib.lib()
    p = PATHS[path]
    m = AC.make(c)
    B, L, H = c["B"], c["L"], c["H"]
    assert int(L_.vo_attention_bwd_workspace_size(B, L, H)) == 4 * m["ws"].numel()
    d = E._dev(m, "qkv", "dout", "lens", "dqkv_buf", "ws_buf")
    with E._Knobs(p["cfg"], xcd):
        if chained:
            o_in, lse = ops.attention(d["qkv"], d["lens"], H, with_lse=True)
        else:
            rf = ref_fwd(dk, c)
            o_in, lse = rf["o_in"].cuda(), rf["lse_in"].cuda()
        o_keep = o_in.clone()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (E._vp(d["qkv"]), E._vp(o_in), E._vp(d["dout"]), ops.vo_dtype(d["qkv"]), E._vp(d["lens"]), B, L, H, dk,
                1.0 / dk ** 0.5)
        tail = (E._vp(E._view(d["dqkv_buf"], m["dqkv"])), E._vp(E._view(d["ws_buf"], m["ws"])), st)
        if p["lse"]:
            _lib.check(L_.vo_attention_bwd_lse(*head, E._vp(lse), *tail), "vo_attention_bwd_lse")
        else:
            _lib.check(L_.vo_attention_bwd(*head, *tail), "vo_attention_bwd")
        torch.cuda.synchronize()
    it = AC._INT[o_in.dtype]
    assert torch.equal(o_in.view(it), o_keep.view(it)), f"{c['name']}: the input o_in changed"
    m["dqkv_buf"].copy_(d["dqkv_buf"].cpu())
    m["ws_buf"].copy_(d["ws_buf"].cpu())
    m["after"] = dict(qkv=d["qkv"].cpu(), dout=d["dout"].cpu())
    return m, o_in.cpu()


@pytest.mark.parametrize("dk,path,c", CASES, ids=_IDS)
def test_attention_heads_edge(head_size, dk, path, c):
    """Every element within its bar, guards and inputs untouched; the forward with and without lse bit-identical
    (E.run_fwd); utterances with no key exact zero rows and +inf lse, masked keys exactly zero dK / dV."""
    head_size(dk)
    if c["kind"] == "fwd":
        m = E.run_fwd(path, c)
        AC.verify(c, m, ref_fwd(dk, c), after=m["after"])
    else:
        m, _ = run_bwd(dk, path, c)
        AC.verify(c, m, ref_bwd(dk, c), after=m["after"])
    E._exact_zero_rows(c, m)


@pytest.mark.parametrize("path", [p for p, d in PATHS.items() if d["kind"] == "bwd"])
@pytest.mark.parametrize("dk", list(HEADS))
def test_attention_heads_bwd_chained(head_size, dk, path):
    """The production pairing: the backward consumes the GPU forward's own out and lse; the reference is
    the float64 backward at that out."""
    head_size(dk)
    c = AC.case(*chained(dk), draw="flat", dt=PATHS[path]["dt"], kind="bwd")
    m, o_in = run_bwd(dk, path, c, chained=True)
    AC.verify(c, m, AC.reference_bwd(c, m, o_in), after=m["after"])


def _outputs(dk, path, c, xcd=0):
    if c["kind"] == "fwd":
        m = E.run_fwd(path, c, xcd)
        return [m["out"].view(AC._INT[m["out"].dtype]), m["lse"].view(torch.int32)]
    m, _ = run_bwd(dk, path, c, xcd)
    return [m["dqkv"].view(AC._INT[m["dqkv"].dtype])]


@pytest.mark.parametrize("which", [0, 1], ids=["L129_Hodd", "L193"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dk", list(HEADS))
def test_attention_heads_xcd_remap_is_bit_identical(head_size, dk, path, which):
    """att_xcd 1 (plain workgroup order) against att_xcd 0: the remap only relabels workgroups."""
    head_size(dk)
    c = AC.case(*identity(dk)[which], draw="flat", dt=PATHS[path]["dt"], kind=PATHS[path]["kind"])
    for a, b in zip(_outputs(dk, path, c, 0), _outputs(dk, path, c, 1)):
        assert torch.equal(a, b), c["name"]


@pytest.mark.parametrize("which", [0, 1], ids=["L129_Hodd", "L193"])
@pytest.mark.parametrize("dk", list(HEADS))
def test_attention_heads_bwd_cfg2_is_bit_identical(head_size, dk, which):
    """attn2_bwd_dkdv_kernel<2, DK> against <0, DK>: the same operations in the same order."""
    head_size(dk)
    c = AC.case(*identity(dk)[which], draw="flat", dt="bf16", kind="bwd")
    assert torch.equal(_outputs(dk, "B3", c)[0], _outputs(dk, "B3x", c)[0]), c["name"]
