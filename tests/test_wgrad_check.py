"""CPU self-test of the weight-gradient checker (tests/wgrad_check.py) and the static checks of the GPU matrix
(tests/test_gpu_wgrad_edges.py): the checker must accept a plain fp32 stand-in on the guarded operands and
reject each deliberate fault by name; every case's declared launch record must be what vo_conv1d_wgrad_plan
returns (host code, no GPU), and the cases together must reach every shipped kernel and path (REQUIRED)."""

import ctypes

import pytest

import test_gpu_wgrad_edges as M
import wgrad_check as WC

_cache = {}


def _prepared(c):
    """(m, ref) of a case with fresh output sets; operands and reference computed once per case."""
    if c["name"] not in _cache:
        m = WC.make(c)
        _cache[c["name"]] = (m, WC.reference(c, m))
    m, ref = _cache[c["name"]]
    m = dict(m, a_buf=m["a_orig"].clone(), b_buf=m["b_orig"].clone(),
             outs=[WC.fresh_out(c, m["ws_floats"]) for _ in range(2)])
    return m, ref


def _check(c, mutate=None):
    m, ref = _prepared(c)
    WC.standin(c, m, mutate)
    return WC.verify(c, m, ref)


def test_case_names_are_unique():
    names = [c["name"] for c in M.CASES]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)


def test_checker_accepts_the_fp32_standin_on_every_gpu_case():
    """The element bar is a worst-case bound: an fp32 sum in utterance order sits far below it (measured 0.002
    at R = 262..1161; 0.05 allows 25 times that)."""
    worst = 0.0
    for c in M.CASES:
        ratio, rel = _check(c)
        worst = max(worst, ratio)
        assert ratio <= 0.05 and rel < 1e-6, (c["name"], ratio, rel)
    print(f"worst error/bar of the stand-in over {len(M.CASES)} cases: {worst:.3e}")


@pytest.mark.parametrize("mutate", sorted(WC.MUTATIONS))
def test_checker_rejects_mutation_by_name(mutate):
    """Every case of the GPU matrix the fault applies to (at least three): verify names the expected failure."""
    cases = [c for c in M.CASES if WC.applies(c, mutate)]
    assert len(cases) >= 3, mutate
    for c in cases:
        with pytest.raises(AssertionError, match=f"{c['name']}: {WC.MUTATIONS[mutate]}: "):
            _check(c, mutate)


@pytest.mark.parametrize("mutate", ["drop_row", "leak_row", "shift_tap"])
def test_boundary_faults_pass_the_old_bf16_bar_and_fail_the_checker(mutate):
    """The whole-tensor 1e-2 bar of the bf16 tests this checker supersedes accepts a fault on a handful of rows
    at an utterance boundary; the element bar does not, on most elements of the tap."""
    passed_old = 0
    for c in M.CASES:
        if c["dt"] != "bf16" or not WC.applies(c, mutate):
            continue
        m, ref = _prepared(c)
        WC.standin(c, m, mutate)
        old = WC.old_bf16_rel_l2(c, m, ref)
        with pytest.raises(AssertionError, match="element bar"):
            WC.verify(c, m, ref)
        passed_old += old < WC.OLD_BF16_REL_L2
    assert passed_old >= 1, mutate


def test_drop_row_fails_most_elements_of_its_tap():
    c = next(c for c in M.CASES if c["name"] == "bf16_B3_T107_M64_N64_K3_p1_preb")
    m, ref = _prepared(c)
    WC.standin(c, m, "drop_row")
    got = WC.dw_view(c, m["outs"][0]["dw_buf"]).double()
    over = ((got - ref["dw"]).abs() > ref["dw_bar"])[:, :, c["K"] - 1].double().mean()
    assert float(over) > 0.8, float(over)


def test_every_declared_record_is_the_plan():
    """vo_conv1d_wgrad_plan (no kernel launched, the knobs of the case set) returns exactly the record the case
    declares, and the knobs are back at 0 afterwards."""
    from visual_onoma_to_wave_amd import _lib, ops
    for c in M.CASES:
        args, kw = WC.plan_args(c)
        with WC.knobs(c):
            got = ops.conv1d_wgrad_plan(*args, **kw)
        assert got == WC.record(c), (c["name"], got, WC.record(c))
        assert c["B"] * c["T_A"] <= WC.R_MAX
    assert all(_lib.lib().vo_tune_get(k) == 0 for k in (b"wgrad_cfg", b"wgrad_kg", b"wgrad_mt"))
    assert tuple(ops.WGRAD_LAUNCH_FIELDS) == WC.FIELDS


def test_matrix_reaches_every_required_instantiation_and_path():
    reached = set().union(*(WC.reached(c) for c in M.CASES))
    missing = sorted(map(str, M.REQUIRED - reached))
    assert not missing, missing
    assert len({r for r in M.REQUIRED if isinstance(r, tuple)}) == 51


def test_rejected_wgrad_leaves_a_zero_record():
    """Host side of vo_conv1d_wgrad_last_launch / _plan: every call here is refused by the argument checks before
    any device work.  A refused call reads as zeros, the copies are clamped to n, the field count is pinned, and
    a refused plan returns -1 with a zero record and leaves the last-launch record alone."""
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    P = 4096  # never dereferenced
    assert L.vo_conv1d_wgrad_bias(P, 64, 16, P, 64, 16, 2, 60, 64, 3, 1, 1, 1, 1, 0, 0, 0.0, _lib.VO_BF16, P, None, P,
                                  None) == -1
    assert b"multiples of 8" in L.vo_last_error()
    assert set(ops.conv1d_wgrad_last_launch().values()) == {0}
    assert len(ops.WGRAD_LAUNCH_FIELDS) == 12
    rec = (ctypes.c_int32 * 16)(*([7] * 16))
    assert L.vo_conv1d_wgrad_last_launch(rec, 3) == 3 and list(rec[:4]) == [0, 0, 0, 7]
    assert L.vo_conv1d_wgrad_last_launch(rec, 64) == 12 and list(rec[11:13]) == [0, 7]
    assert L.vo_conv1d_wgrad_last_launch(None, 12) == 0
    # the fused bias with pre_a, split-bf16 with a stride: refused by the launch and by the plan alike
    assert L.vo_conv1d_wgrad_bias(P, 64, 16, P, 64, 16, 2, 64, 64, 3, 1, 1, 1, 1, 1, 0, 0.1, _lib.VO_BF16, P, P, P,
                                  None) == -1
    rec = (ctypes.c_int32 * 16)(*([7] * 16))
    assert L.vo_conv1d_wgrad_plan(2, 16, 16, 64, 64, 3, 1, 1, 1, 1, 1, 0, _lib.VO_BF16, 1, rec, 12) == -1
    assert b"pre_a" in L.vo_last_error() and list(rec[:13]) == [0] * 12 + [7]
    with pytest.raises(RuntimeError, match="F32X3"):
        ops.conv1d_wgrad_plan(2, 16, 31, 64, 64, 3, S=2, pad=1, dtype=_lib.VO_F32X3)
    rec = (ctypes.c_int32 * 16)(*([7] * 16))
    assert L.vo_conv1d_wgrad_plan(2, 16, 16, 64, 64, 3, 1, 1, 1, 1, 0, 0, _lib.VO_BF16, 0, rec, 3) == 0
    assert list(rec[:4]) == [WC.PER_TAP, 64, 0, 7]
    assert L.vo_conv1d_wgrad_plan(2, 16, 16, 64, 64, 3, 1, 1, 1, 1, 0, 0, _lib.VO_BF16, 0, None, 12) == 0
    assert set(ops.conv1d_wgrad_last_launch().values()) == {0}
