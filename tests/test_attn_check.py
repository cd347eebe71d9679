"""CPU self-test of the attention checker (tests/attn_check.py) and the static coverage check of the GPU
matrix (tests/test_gpu_attention_edges.py).  Accept: the CPU emulation of the kernels' arithmetic passes
verify on every case of the matrix in both dtypes -- the condition that a correct kernel can pass every
case.  Reject: each deliberate fault raises in verify."""

import pytest

import attn_check as AC
import test_gpu_attention_edges as M

# the matrix's cases without their paths, in both dtypes
_UNIQ = {}
for _p, _c in M.CASES:
    for _dt in ("f32", "bf16"):
        _k = AC.case(_c["B"], _c["L"], _c["H"], _c["lens"], draw=_c["draw"], dt=_dt, kind=_c["kind"])
        _UNIQ[_k["name"]] = _k
ALL = list(_UNIQ.values())
SMALL = [c for c in ALL if c["L"] <= 129]

_REFS = {}


def _fwd_ref(c):
    k = AC.case(c["B"], c["L"], c["H"], c["lens"], draw=c["draw"], dt=c["dt"], kind="fwd")
    if k["name"] not in _REFS:
        _REFS[k["name"]] = AC.reference_fwd(k, AC.make(k))
    return _REFS[k["name"]]


def _bwd_ref(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = AC.reference_bwd(c, AC.make(c), _fwd_ref(c)["o_in"])
    return _REFS[c["name"]]


def _check(c, mutate=None):
    m = AC.make(c)
    rf = _fwd_ref(c)
    if c["kind"] == "fwd":
        AC.emulate_fwd(c, m, mutate)
        return AC.verify(c, m, rf)
    AC.emulate_bwd(c, m, rf["o_in"], rf["lse_in"], mutate)
    return AC.verify(c, m, _bwd_ref(c))


_WORST = {}


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_checker_accepts_emulation(c):
    ratio, rel = _check(c)
    key = (c["kind"], c["dt"])
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print(f"worst error/bar so far {key}: {_WORST[key]:.3f}")
    assert ratio <= 1.0


def _mutants(kind, names):
    out = []
    for c in SMALL:
        if c["kind"] == kind:
            out += [(c, mu) for mu in names if AC.applies(c, mu)]
    return out


_FWD = _mutants("fwd", AC.FWD_MUTATIONS)
_BWD = _mutants("bwd", AC.BWD_MUTATIONS)


@pytest.mark.parametrize("c,mutate", _FWD + _BWD, ids=[f"{mu}-{c['name']}" for c, mu in _FWD + _BWD])
def test_checker_rejects_mutation(c, mutate):
    with pytest.raises(AssertionError):
        _check(c, mutate)


def test_every_mutation_has_cases():
    """applies() leaves out only what a mutation cannot change: every mutation still meets every dtype, most
    shapes and every draw but those attn_check.BLIND names."""
    for kind, pairs, names in (("fwd", _FWD, AC.FWD_MUTATIONS), ("bwd", _BWD, AC.BWD_MUTATIONS)):
        n_kind = len([c for c in SMALL if c["kind"] == kind])
        for mu in names:
            cs = [c for c, x in pairs if x == mu]
            assert {c["dt"] for c in cs} == {"f32", "bf16"}, mu
            assert len(cs) >= (n_kind * 3 // 10 if mu == "no_rescale" else n_kind * 7 // 10), (mu, len(cs), n_kind)
            draws = set(AC.DRAWS) - AC.BLIND.get(mu, set())
            assert {c["draw"] for c in cs} == draws, mu


def test_zero_pad_keys_rejected_on_the_peaked_draw():
    """The defect attention_kernel had (keys [L, 64 ceil(L / 64)) admitted with score 0 when lens > L) moves a
    peaked softmax by 1e-5 .. 7e-4 in rel-L2: no whole-tensor bar sees it, the element bar does."""
    for dt in ("f32", "bf16"):
        c = AC.case(2, 65, 2, [200, 66], draw="peaked", dt=dt, kind="fwd")
        assert c["name"] in _UNIQ and AC.applies(c, "zero_pad_keys")
        with pytest.raises(AssertionError, match="over the bar"):
            _check(c, "zero_pad_keys")


def test_matrix_coverage():
    """Every path against every shape of the first list and every draw; lens = None, lens > L and lens = 0 for
    every path; the chained and bit-identity cases use shapes of the matrix."""
    assert set(M.PATHS) == {"F1", "F2", "F3", "B1", "B2", "B2L", "B3", "B3x"}
    assert len(M.SHAPES) == 10
    have = {(p, c["B"], c["L"], c["H"], None if c["lens"] is None else tuple(c["lens"]), c["draw"]) for p, c in M.CASES}
    for p, d in M.PATHS.items():
        for B, L, H, lens in M.SHAPES + M.LENS_OVER + [M.LENS_ZERO, M.LENS_NEGATIVE]:
            assert (p, B, L, H, None if lens is None else tuple(lens), "flat") in have, (p, L)
        for draw in AC.DRAWS:
            assert {L for q, _, L, _, _, dr in have if q == p and dr == draw} >= {65, 129, 193}, (p, draw)
        mine = [c for q, c in M.CASES if q == p]
        assert all(c["dt"] == d["dt"] and c["kind"] == d["kind"] for c in mine)
        assert any(c["lens"] is None for c in mine)
        assert any(c["lens"] and max(c["lens"]) > c["L"] for c in mine)
        assert any(c["lens"] and min(c["lens"]) == 0 for c in mine)
        assert any(c["draw"] == "peaked" and c["L"] == 1000 for c in mine)
    assert M.CHAINED in M.SHAPES and all(s in M.SHAPES for s in M.IDENTITY)


@pytest.mark.parametrize("dt,tol", [("f32", 4e-8), ("bf16", 2.7e-3)])
@pytest.mark.parametrize("draw", ["flat", "peaked"])
def test_reference_matches_float64_autograd(draw, dt, tol):
    """The references against torch's own float64 softmax and autograd: the forward to rounding, the backward
    exactly when handed the exact O, and within the docstring's figures when handed O rounded to the dtype."""
    import torch
    c = AC.case(2, 193, 2, [130, 193], draw=draw, dt=dt, kind="bwd")
    m = AC.make(c)
    x = m["qkv"].double().requires_grad_()
    q, k, v = (t.reshape(2, 193, 2, 128).transpose(1, 2) for t in x.split(256, dim=-1))
    s = q @ k.transpose(-1, -2) / 128 ** 0.5
    mask = torch.arange(193)[None, None, None, :] >= torch.tensor(c["lens"])[:, None, None, None]
    o = (torch.softmax(s.masked_fill(mask, -float("inf")), dim=-1) @ v).transpose(1, 2).reshape(2, 193, 256)
    o.backward(m["dout"].double())
    rf = AC.reference_fwd(c, m)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    assert rel(rf["out"], o.detach()) < 1e-13
    assert rel(AC.reference_bwd(c, m, rf["out"])["dqkv"], x.grad) < 1e-12
    assert rel(AC.reference_bwd(c, m, rf["o_in"])["dqkv"], x.grad) <= tol


def test_make_draws():
    """The draws do what the cases rely on: dtype-exact operands, the peaked draw's p_max, the ramps' tile
    maxima, the poison where and only where no key is."""
    import torch
    c = AC.case(2, 193, 2, [130, 193], draw="peaked", dt="bf16")
    m = AC.make(c)
    assert torch.equal(m["qkv"].float().bfloat16(), m["qkv"])
    _, _, _, Q, K, _ = next(AC._heads(c, m))
    P = AC._probs(Q, K, 130)[1]
    assert 0.3 < float(P.max(dim=1).values.mean()) < 0.7
    for draw, sign in (("ramp_up", 1), ("ramp_down", -1)):
        c = AC.case(2, 193, 2, [130, 193], draw=draw, dt="f32")
        b, h, n, Q, K, _ = list(AC._heads(c, AC.make(c)))[2]
        S = AC._probs(Q, K, n)[0]
        tmax = torch.stack([S[:, t * 64:(t + 1) * 64].max(dim=1).values for t in range(3)], dim=1)
        step = (tmax[:, 1:] - tmax[:, :-1]) * sign
        assert 4 < float(step.mean()) < 12 and float((S.max(dim=1).values - S.min(dim=1).values).max()) < 80
    c = AC.case(3, 65, 2, [65, 64, 1], draw="poison_pad", dt="bf16")
    m = AC.make(c)
    kv = m["qkv"][:, :, 256:].float().abs()
    assert bool((kv[1, 64:] == AC.POISON).all()) and bool((kv[2, 1:] == AC.POISON).all())
    assert float(kv[0].max()) < 10 and float(kv[1, :64].max()) < 10
    assert float(m["qkv"][:, :, :256].float().abs().max()) < 10
