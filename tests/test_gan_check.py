"""CPU self-test of the GAN loss-term checker (tests/gan_check.py) on the cases of tests/test_gpu_gan_terms.py: it
must accept a plain fp32 stand-in and reject each deliberate fault by name, and a dropped or doubled unit must
exceed the sum bar by gan_check.FACTOR wherever the case claims it."""

import pytest

import gan_check as GC
import test_gpu_gan_terms as M

# the two cases past the gradient's grid cap (tens of MB of buffers) are checked once, unmutated, in bf16
SMALL = [c for c in M.CASES if not c["grad_cap"]]
_cache = {}


def _prepared(c):
    """(m, ref) with fresh operand copies and output sets; operands and reference drawn once per case."""
    if c["name"] not in _cache:
        m = GC.make(c)
        _cache[c["name"]] = (m, GC.reference(c, m))
    m, ref = _cache[c["name"]]
    m = dict(m, a_buf=[x.clone() for x in m["a_orig"]], b_buf=[None if x is None else x.clone() for x in m["b_orig"]],
             outs=[GC.fresh_out(c, m["ws_floats"]) for _ in range(2)])
    return m, ref


def _check(c, mutate=None):
    m, ref = _prepared(c)
    GC.run(c, m, GC.Standin(c, m, mutate))
    return GC.verify(c, m, ref), m, ref


def test_case_names_are_unique():
    names = [c["name"] for c in M.CASES]
    assert len(set(names)) == len(names)


def test_workspace_size_is_512_floats_per_term_of_a_table():
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    assert [int(L.vo_gan_reduce_multi_workspace_size(n)) for n in (1, 32, 33)] == [2048, 65536, 65536]


def test_cases_cover_the_paths():
    """Both unit widths at every unit count the issue names, the misaligned base on the scalar path for bf16 only,
    a table of 32 and one of 33 terms mixing both widths and all three kinds."""
    for dt in ("bf16", "f32"):
        seen = {(GC.chain(c, t)[0], GC.chain(c, t)[1]) for c in M.CASES if c["dt"] == dt for t in c["terms"]}
        for V in (1, 8):
            for u in (1, 255, 256, 257, 512 * 256 + 1, 4096 * 256 + 1):
                assert (V, u) in seen, (dt, V, u)
        off4 = next(c for c in M.CASES if c["name"] == f"{dt}_w64_off4")
        assert GC.vec8(off4, off4["terms"][0]) == (dt == "f32")
        for n in (32, 33):
            c = next(c for c in M.CASES if c["name"] == f"{dt}_terms{n}")
            assert len(c["terms"]) == n
            assert {(GC.vec8(c, t), t["kind"]) for t in c["terms"]} == {(v, k) for v in (True, False) for k in range(3)}


def test_checker_accepts_the_fp32_standin():
    """The bar is a worst-case bound; torch's pairwise fp32 sum sits far below it."""
    worst = 0.0
    for c in SMALL:
        worst = max(worst, _check(c)[0])
    assert worst <= 0.25, worst


def test_checker_accepts_the_standin_past_the_gradient_grid_cap():
    for c in M.CASES:
        if c["grad_cap"] and c["dt"] == "bf16":
            m = GC.make(c)
            GC.run(c, m, GC.Standin(c, m))
            GC.verify(c, m, GC.reference(c, m))


@pytest.mark.parametrize("mutate", sorted(GC.MUTATIONS))
def test_checker_rejects_mutation_by_name(mutate):
    cases = [c for c in SMALL if GC.applies(c, mutate)]
    assert len(cases) >= 3, mutate
    for c in cases:
        with pytest.raises(AssertionError, match=f"{c['name']}: {GC.MUTATIONS[mutate]}: ".replace("+", r"\+")):
            _check(c, mutate)


@pytest.mark.parametrize("mutate", ["drop_unit", "double_unit"])
def test_a_dropped_or_doubled_unit_exceeds_the_sum_bar_by_the_stated_factor(mutate):
    for c in SMALL:
        m, ref = _prepared(c)
        GC.run(c, m, GC.Standin(c, m, mutate))
        got = float(m["outs"][0]["sum_single"][GC.GUARD_N])
        assert abs(got - ref["S"][0]) >= GC.FACTOR * ref["bar"][0], (c["name"], got, ref["S"][0], ref["bar"][0])
