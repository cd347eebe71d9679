"""CPU self-test of the normalisation checker (tests/norm_check.py) and the static checks of the GPU matrix
(tests/test_gpu_norm_edges.py): the checker must accept a plain fp32 stand-in on the guarded operands and reject
each deliberate fault by name; every BatchNorm case's declared route record must be what vo_bn_route returns
(host code, no GPU); the cases together must reach every shipped instantiation and edge (REQUIRED)."""

import ctypes

import pytest
import torch

import norm_check as NC
import test_gpu_norm_edges as M

_cache = {}


def _prepared(c):
    """(m, ref) of a case with fresh buffers; operands and reference computed once per case."""
    if c["name"] not in _cache:
        from visual_onoma_to_wave_amd import _lib
        m = NC.make(c)
        if c["kind"] == "bn":
            NC.add_workspace(c, m, int(_lib.lib().vo_bn_workspace_size(c["M"], c["C"])))
        _cache[c["name"]] = (m, NC.reference(c, m))
    m, ref = _cache[c["name"]]
    return NC.fresh(m), ref


def _check(c, mutate=None, report=None):
    m, ref = _prepared(c)
    NC.standin(c, m, mutate)
    return NC.verify(c, m, ref, report)


def test_case_names_are_unique():
    names = [c["name"] for c in M.CASES]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert all(c["M"] * c["C"] * 4 <= 2 ** 22 for c in M.BN_CASES)
    assert all(c["B"] * c["T"] * c["D"] * 4 <= 2 ** 23 for c in M.LN_CASES)


def test_checker_accepts_the_fp32_standin_on_every_gpu_case():
    """The bars are worst-case bounds.  The stand-in's fp32 outputs sit far below them, measured here: LayerNorm 0.009
    on y, 0.009 on gh / gres, 0.05 on dgamma / dbeta; BatchNorm 0.09 on y, 0.14 on dx and 0.09 on dgamma / dbeta (both
    at M <= 9, where the bar is a few ulp), 0.26 on the statistics of a constant channel and of M = 1 (rstd =
    eps^-1/2: fp32 rounds eps itself, one ulp of a four-ulp bar).  0.3 covers those.  bf16 outputs and the FLAT
    backward's rounded-once outputs come within a hair of their half-ulp term by construction; for them the check
    is the bar itself, which verify applies."""
    worst = 0.0
    for c in M.CASES:
        rep = {}
        _check(c, report=rep)
        flat = c["kind"] == "bn" and NC.record(c, "bwd")["route"] == NC.FLAT
        for k, ratio in rep.items():
            m = _cache[c["name"]][0]
            if NC.view(m, k).dtype == torch.bfloat16 or (flat and k in ("dx", "dgamma", "dbeta")):
                continue
            worst = max(worst, ratio)
            assert ratio <= 0.3, (c["name"], k, ratio)
    print(f"worst error/bar of the stand-in's fp32 outputs over {len(M.CASES)} cases: {worst:.3e}")


def test_standin_rel_l2_of_ill_conditioned_cases_is_as_recorded():
    """STANDIN_REL_L2 (the whole-tensor bar of the offset / constant cases is 4 x these) holds what the stand-in
    reaches here, within a factor 1.5 (the order of torch's fp32 reductions depends on the CPU's vector width; on
    the machine that measured them the match is to the printed digits); prints the table in the form the GPU file
    holds it."""
    lines = []
    for c in M.CASES:
        if NC.well_conditioned(c):
            assert c["ill"] is None, c["name"]
            continue
        m, ref = _prepared(c)
        NC.standin(c, m)
        got = {k: NC.rel_l2(NC.view(m, k).double(), ref[k][0]) for k in ref if k in NC.WHOLE}
        lines.append(f'    "{c["name"]}": {{' + ", ".join(f'"{k}": {v:.3e}' for k, v in got.items()) + "},")
        assert c["ill"] is not None and set(c["ill"]) == set(got), c["name"]
        for k, v in got.items():
            assert c["ill"][k] / 1.5 - 1e-12 <= v <= c["ill"][k] * 1.5 + 1e-12, (c["name"], k, v, c["ill"][k])
    print("\n".join(lines))


@pytest.mark.parametrize("mutate", sorted(NC.MUTATIONS))
def test_checker_rejects_mutation_by_name(mutate):
    """Every case of the GPU matrix the fault applies to (at least three): verify names the expected failure."""
    cases = [c for c in M.CASES if NC.applies(c, mutate)]
    assert len(cases) >= 3, (mutate, len(cases))
    for c in cases:
        with pytest.raises(AssertionError, match=f"{c['name']}: {NC.MUTATIONS[mutate]}: "):
            _check(c, mutate)


def _by_name(name):
    return next(c for c in M.CASES if c["name"] == name)


def test_a_live_pad_row_passes_the_old_bf16_bar_and_fails_the_checker():
    """One pad row of 513 normalised instead of zeroed, its inputs 0.25 throughout (y = beta on that row): rel-L2
    0.5 %, under the 1e-2 the bf16 tests allowed.  The checker names it, whatever the row holds."""
    c = _by_name("ln_fwd_bf16_bf16_bf16_D256_B9_T57_zero_mid")
    m, ref = _prepared(c)
    for k in ("x", "res"):
        NC.view(m, k)[~m["live"]] = 0.25
    NC.standin(c, m, "pad_row_live")
    old = NC.old_rel_l2(c, m, ref)
    assert 1e-3 < old < NC.OLD_BF16_REL_L2, old
    for k in ("x", "res"):
        m["bufs"][k] = m["orig"][k].clone()
    with pytest.raises(AssertionError, match=f"{c['name']}: pad row: "):
        NC.verify(c, m, ref)


def test_a_dropped_partial_passes_the_old_bf16_bar_and_fails_the_checker():
    """The last workgroup's partial (one live row of 820, its gy at 1 / 8 of the others') left out of dgamma / dbeta:
    rel-L2 (1 / 8) / sqrt(820) = 0.4 %, under the old 1e-2; the element bar, 2 (R + 8) u sum|term| = 0.05 here,
    catches every column whose term of that row is larger."""
    c = _by_name("ln_bwd_bf16_bf16_bf16_D256_B5_T205_zero_mid")
    m = NC.make(c)
    NC.view(m, "gy")[-1] *= 0.125
    m["orig"]["gy"] = m["bufs"]["gy"].clone()
    ref = NC.reference(c, m)
    NC.standin(c, m, "drop_partial")
    old = NC.old_rel_l2(c, m, ref)
    assert 1e-3 < old < NC.OLD_BF16_REL_L2, old
    with pytest.raises(AssertionError, match=f"{c['name']}: element bar: "):
        NC.verify(c, m, ref)
    over = (NC.view(m, "dgamma").double() - ref["dgamma"][0]).abs() > ref["dgamma"][1]
    assert float(over.double().mean()) > 0.2, float(over.double().mean())


def test_one_pass_variance_passes_the_old_bar_on_plain_data_and_fails_the_checker_on_offset_rows():
    """E[x^2] - mean^2 in fp32 is as good as two passes on the zero-mean data the old tests drew (rel-L2 < 1e-5 on
    every plain fp32 case), so nothing noticed it; on rows and channels whose mean is 10^3 spreads it is rejected."""
    plain = [c for c in M.CASES if c["profile"] == "plain" and c["tx"] == "f32" and
             (c["kind"] == "bn" or not c["bwd"] and c["t3"] == "f32")]
    assert len(plain) >= 3
    for c in plain:
        m, ref = _prepared(c)
        NC.standin(c, m, "one_pass_var")
        assert NC.rel_l2(NC.view(m, "y").double(), ref["y"][0]) < NC.REL_L2_F32, c["name"]
    hit = [c for c in M.CASES if NC.applies(c, "one_pass_var")]
    assert len(hit) >= 3
    for c in hit:
        with pytest.raises(AssertionError, match=f"{c['name']}: {NC.MUTATIONS['one_pass_var']}: "):
            _check(c, "one_pass_var")


def test_nan_in_a_pad_row_zero_is_pinned():
    """lens[0] == 0 with NaN in batch 0's rows of x, res, gy and gy2, row 0 among them -- the row a dead row of the
    backward kernel loads in its own place: such cases exist for the plain, the _ex and the _drop entry."""
    for entry in ("bwd", "bwd_ex", "bwd_drop"):
        cs = [c for c in M.LN_CASES if c["entry"] == entry and c["lens"] == "zero_first"]
        assert cs, entry
        for c in cs:
            m, _ = _prepared(c)
            assert NC.lens_of(c)[0] == 0 and not bool(m["live"][0])
            for k in ("x", "res", "gy", "gy2"):
                if k in m["spec"]:
                    assert bool(torch.isnan(NC.view(m, k)[0].float()).all()), (c["name"], k)


def test_every_declared_record_is_the_route():
    """vo_bn_route (no launch, no GPU call) returns the record every BatchNorm case declares, forward and backward;
    a misaligned case declares the scalar route; C = 12 fp32 applies with a multiple of 3 blocks."""
    from visual_onoma_to_wave_amd import ops
    assert tuple(ops.BN_ROUTE_FIELDS) == NC.BN_FIELDS
    assert (ops.BN_SCALAR, ops.BN_VEC, ops.BN_FLAT) == (NC.SCALAR, NC.VEC, NC.FLAT)
    for c in M.BN_CASES:
        for which in ("fwd", "bwd"):
            got = ops.bn_route(*NC.route_args(c, which))
            assert got == NC.record(c, which), (c["name"], which, got)
            if c["misaligned"]:
                assert got["route"] == NC.SCALAR, c["name"]
            if c["C"] == 12 and c["tx"] == "f32":
                assert got["route"] == NC.VEC and got["apply_blocks"] % 3 == 0
    assert sum(c["misaligned"] for c in M.BN_CASES) >= 3


def test_matrix_reaches_every_required_instantiation_and_edge():
    reached = set().union(*(NC.reached(c) for c in M.CASES))
    missing = sorted(map(str, M.REQUIRED - reached))
    assert not missing, missing
    assert len({r for r in M.REQUIRED if isinstance(r, tuple) and r[0].startswith("layernorm")}) == 58
    assert len({r for r in M.REQUIRED if isinstance(r, tuple) and r[0].startswith("bn_")}) == 43


def test_every_accepted_layernorm_call_is_run_by_a_case():
    """NC.LN_ACCEPTS against the GPU matrix: every call an entry takes -- that entry, those dtypes, with or without
    y16 / gy2 / gh32 -- is the C call of some case of CASES (``reached``, at either NPL), so the accepted side of the
    table is run and checked per element, and no case makes a call outside the table; every accepted call lies in
    its entry's domain (the refusal test walks the rest); the table names 16 forward and 12 backward kernels."""
    assert set(NC.LN_ACCEPTS) == set(NC.LN_ENTRIES)
    ran = {r[1:] for c in M.LN_CASES for r in NC.reached(c) if isinstance(r, tuple) and r[0] == "ln_call"}
    assert ran == {(e,) + combo for e, combos in NC.LN_ACCEPTS.items() for combo in combos}
    inst = set()
    for entry, combos in NC.LN_ACCEPTS.items():
        assert combos <= set(NC.ln_domain(entry)), entry
        for combo in combos:
            assert (entry,) + combo in ran, (entry, combo)
            inst |= {NC.ln_instantiation(entry, combo) + (npl,) for npl in (4, 8)}
    assert sum(i[0] == "layernorm_kernel" for i in inst) == 16
    assert sum(i[0] == "layernorm_bwd_kernel" for i in inst) == 12
    assert sum(len(NC.ln_domain(e)) - len(NC.LN_ACCEPTS[e]) for e in NC.LN_ENTRIES) == 46


def test_bn_route_alignment_rule_and_rejections():
    """Host side of vo_bn_route: 16-byte alignment of x, dy and the output on the vectorised and FLAT routes (8 bytes
    for a bf16 dy beside an fp32 x), null pointers meaning aligned, the bf16 x / fp32 dy exception, the clamped
    copy, and refused sizes."""
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    f32, bf16 = torch.float32, torch.bfloat16
    A = 1 << 20
    assert ops.bn_route(64, 512, bf16)["route"] == NC.VEC
    assert ops.bn_route(64, 512, bf16, bf16, A, A, A)["route"] == NC.VEC
    for bad in ((A + 2, A, A), (A, A + 8, A), (A, A, A + 4)):
        assert ops.bn_route(64, 512, bf16, bf16, *bad)["route"] == NC.SCALAR, bad
    assert ops.bn_route(64, 512, bf16, None, A, None, A + 8)["route"] == NC.SCALAR
    assert ops.bn_route(64, 512, bf16, f32, A, A, A)["route"] == NC.SCALAR       # no vector form
    assert ops.bn_route(64, 512, f32, bf16, A, A + 8, A)["route"] == NC.VEC       # dy read 8 bytes at a time
    assert ops.bn_route(64, 512, f32, bf16, A, A + 4, A)["route"] == NC.SCALAR
    assert ops.bn_route(64, 512, f32, f32, A, A + 8, A)["route"] == NC.SCALAR
    assert ops.bn_route(60, 1, f32, None, A + 60, None, A)["route"] == NC.SCALAR  # x[1:] of an (N, 1, 5, 3) map
    assert ops.bn_route(60, 1, f32, None, A + 64, None, A)["route"] == NC.FLAT
    assert ops.bn_route(61, 1, f32)["route"] == NC.SCALAR and ops.bn_route(2056, 2056, bf16)["route"] == NC.SCALAR
    rec = (ctypes.c_int32 * 12)(*([7] * 12))
    assert L.vo_bn_route(64, 512, _lib.VO_BF16, -1, None, None, None, rec, 3) == 3 and list(rec[:4]) == [1, 8, 64, 7]
    assert L.vo_bn_route(64, 512, _lib.VO_BF16, -1, None, None, None, rec, 64) == 8 and list(rec[7:9]) == [0, 7]
    assert L.vo_bn_route(64, 512, _lib.VO_BF16, -1, None, None, None, None, 8) == 0
    rec = (ctypes.c_int32 * 12)(*([7] * 12))
    assert L.vo_bn_route(0, 512, _lib.VO_BF16, -1, None, None, None, rec, 8) == -1
    assert b"bn_route" in L.vo_last_error() and list(rec[:9]) == [0] * 8 + [7]
    assert L.vo_bn_route(64, 512, 5, -1, None, None, None, rec, 8) == -1
    assert L.vo_bn_route(64, 512, _lib.VO_F32, 7, None, None, None, rec, 8) == -1
    with pytest.raises(RuntimeError, match="bn_route"):
        ops.bn_route(64, 0, f32)
