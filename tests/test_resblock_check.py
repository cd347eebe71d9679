"""CPU self-test of the fused-ResBlock checker (tests/resblock_check.py): the stand-in passes every case of the GPU
matrix with its worst row value at or under 5e-3, every mutation is rejected with the right failure named, the
boundary mutations pass the earlier whole-tensor bar and fail the checker, and the matrix reaches every shipped
dense route."""
import pytest
import torch
import torch.nn.functional as F

import resblock_check as RC
from helpers import rel_l2


def _fixed(name, *_):
    return RC.FIXED_TILE_ROWS[name]


MATRIX = RC.matrix(_fixed)
ROUTES = list(RC.routes())


def _check(c, mutate=None, tile=None):
    m = RC.make(c)
    ref, bar = RC.reference(c, m)
    RC.emulate(c, m, mutate, tile)
    return RC.verify(c, m, ref, bar)


@pytest.mark.parametrize("route", ROUTES)
def test_standin_passes_every_case_of_the_gpu_matrix(route):
    """The unmutated stand-in on the route's cases (tile rows from FIXED_TILE_ROWS, the table of today's library):
    inside the element bar, and at or under STANDIN_ROW_MAX per row -- half the row bar."""
    cases = [c for name, _, c in MATRIX if name == route]
    assert cases
    for c in cases:
        assert c["B"] == 3
        ratio, row = _check(c)
        assert ratio <= 1.0
        assert row <= RC.STANDIN_ROW_MAX, f"{c['name']}: stand-in row value {row:.3e}"


# (case, tile rows): one per entry family, T past one tile so that the faults local to a tile apply
PAIR_CASES = [(RC.case("pair", 3, 1000, 32, 7, (5,), acc="mrf"), 506),
              (RC.case("pair_frag", 3, 520, 128, 11, (1,), acc="add"), 246)]
BLOCK_CASES = [(RC.case("block3", 3, 250, 32, 3, (1, 3, 5), acc="mrf"), 104),
               (RC.case("blockk", 3, 1000, 32, 7, (1, 3, 5), acc="mrf"), 952)]


def _kind(mutate, whole_block):
    """The failure verify must name.  The pairs' element bar is tight (the stand-in reaches 0.9 of it) and comes
    first; the whole-block bar compounds three stages' worst cases, and there the row bar catches the fault."""
    return "guard" if mutate == "guard" else ("row bar" if whole_block else "element bar")


@pytest.mark.parametrize("mutate", [m for m in RC.MUTATIONS if m != "x1_pad"])  # a pair has no x_1
@pytest.mark.parametrize("ci", range(len(PAIR_CASES)))
def test_checker_rejects_mutation_pair(ci, mutate):
    c, tile = PAIR_CASES[ci]
    _check(c)
    with pytest.raises(AssertionError, match=f"{c['name']}: {_kind(mutate, False)}:"):
        _check(c, mutate, tile)


@pytest.mark.parametrize("mutate", RC.MUTATIONS)
@pytest.mark.parametrize("ci", range(len(BLOCK_CASES)))
def test_checker_rejects_mutation_whole_block(ci, mutate):
    c, tile = BLOCK_CASES[ci]
    _check(c)
    with pytest.raises(AssertionError, match=f"{c['name']}: {_kind(mutate, True)}:"):
        _check(c, mutate, tile)


def test_acc_scale_needs_an_accumulator_and_x1_pad_a_second_stage():
    """Where a mutation does not apply it changes nothing: the rejections above are the mutations' own."""
    c = RC.case("pair", 2, 300, 32, 3, (1,))
    base = RC.make(c)
    RC.emulate(c, base)
    for mutate in ("acc_scale", "x1_pad"):
        m = RC.make(c)
        RC.emulate(c, m, mutate)
        assert torch.equal(m["y_buf"].view(torch.int16), base["y_buf"].view(torch.int16))


def _torch_fp32(c, m):
    """The earlier tests' reference: the torch fp32 ResBlock pair on the case's operands, (B, T, C)."""
    (d,), K, s = c["dils"], c["K"], c["slope"]
    xf = m["x_val"].transpose(1, 2)
    t = F.leaky_relu(F.conv1d(F.leaky_relu(xf, s), m["w1"][0], m["b1"][0], padding=d * (K - 1) // 2, dilation=d), s)
    return ((F.conv1d(t, m["w2"][0], m["b2"][0], padding=(K - 1) // 2) + xf) * c["out_scale"]).transpose(1, 2)


@pytest.mark.parametrize("bias_std", [0.1, 0.5])
@pytest.mark.parametrize("mutate", ["t1_pad", "tile_mask", "leak_row"])
def test_boundary_mutations_pass_the_whole_tensor_bar_and_fail_the_checker(mutate, bias_std):
    """The gap this checker closes, at C = 32, K = 3, T = 1000, B = 2: a T1 halo row computed from padding, a T1
    mask applied at the batch's ends only, and a neighbour's row read as halo stay under the whole-tensor
    rel-L2 < 1e-2 of the earlier tests -- with their bias draw (0.1 N(0, 1)) and with the checker's (0.5) -- and fail
    the checker under either draw.
    The seed is fixed at 1 for all six cases.  Over seeds 1-9 and the default one the whole-tensor figures are:
    t1_pad 5.7e-3 to 9.8e-3 (0.1) and 6.8e-3 to 1.2e-2 (0.5: the larger biases alone bring this fault to the edge
    of the old bar, six draws of ten are over it; seed 1 gives 8.8e-3), tile_mask 3.9e-3 to 8.4e-3, leak_row
    3.0e-3 to 7.1e-3.  The checker rejects every one of them."""
    c = RC.case("pair", 2, 1000, 32, 3, (1,), bias_std=bias_std, seed=1)
    m = RC.make(c)
    old_ref = _torch_fp32(c, m)  # this draw's own reference
    ref, bar = RC.reference(c, m)
    RC.emulate(c, m)
    clean = rel_l2(m["y"].float(), old_ref)
    RC.verify(c, m, ref, bar)
    RC.emulate(c, m, mutate)
    whole = rel_l2(m["y"].float(), old_ref)
    print(f"{mutate}, bias std {bias_std}: whole-tensor rel-L2 {whole:.3e} (unmutated {clean:.3e})")
    assert whole > clean
    assert whole < 1e-2
    with pytest.raises(AssertionError, match="element bar"):
        RC.verify(c, m, ref, bar)


def test_matrix_covers_every_shipped_dense_route():
    """Every route of the shipped dispatch, at every length that is an edge for it, in every accumulator mode it
    has: written out by hand here, so that a route dropped from resblock_check.routes() is noticed."""
    required = set()
    for C, Ks in [(32, (3, 7, 11)), (64, (3, 5, 9, 7, 11)), (128, (3, 5, 9, 7, 11))]:
        required |= {("pair", C, K, (d,), None) for K in Ks for d in (1, 5)}
    for C in (64, 128):
        for K in (7, 11):
            required |= {("pair", C, K, (d,), ("pair_cfg", 93)) for d in (1, 5)}
            required |= {("pair_frag", C, K, (d,), None) for d in (1, 5)}
    required |= {("block3", C, 3, (1, 3, 5), None) for C in (32, 64, 128)}
    required |= {("block3", 32, 3, (1, 2, 4), None), ("block3", 32, 3, (1, 3, 5), ("rb3_cfg", 80))}
    required |= {("blockk", 32, K, (1, 3, 5), None) for K in (7, 11)}
    seen = {}
    for name, bt, c in MATRIX:
        key = (c["entry"], c["C"], c["K"], c["dils"], c["knob"])
        seen.setdefault(key, (bt, set(), set()))
        seen[key][1].add(c["T"])
        seen[key][2].add(c["acc"])
    assert set(seen) == required
    for (entry, C, K, dils, knob), (bt, Ts, accs) in seen.items():
        h = (K - 1) // 2
        want = {1, h, h + 1, bt - 1, bt, bt + 1, 2 * bt + 3}
        if entry in ("block3", "blockk"):
            hl = sum((d + 1) * h for d in dils)
            want |= {hl - 1, hl + 1}
        assert Ts == want, (entry, C, K, dils, knob)
        assert accs == ({"none", "mrf"} if entry == "blockk" else {"none", "mrf", "add"})
    assert max(c["T"] for _, _, c in MATRIX) == 2 * 952 + 3  # the longest case: about 1.9 k rows at C = 32


def test_tile_row_queries_match_the_fixed_table():
    """vo_resblock_pair_tile_rows / vo_resblock3_tile_rows (host only: no GPU needed) against FIXED_TILE_ROWS and
    today's values; 0 for a refused shape.  A retiling fails here until the table follows it."""
    from visual_onoma_to_wave_amd import _lib, ops
    for name, (entry, C, K, dil_list, knob, _) in RC.routes().items():
        if knob:
            _lib.lib().vo_tune(knob[0].encode(), knob[1])
        try:
            for dils in dil_list:
                if entry == "blockk":
                    got = ops.resblock_k_tile_rows(K)
                elif entry == "block3":
                    got = ops.resblock3_tile_rows(C, dils)
                else:
                    got = ops.resblock_pair_tile_rows(C, K, dils[0], frag=entry == "pair_frag")
                assert got == RC.FIXED_TILE_ROWS[name], (name, dils, got)
        finally:
            if knob:
                _lib.lib().vo_tune(knob[0].encode(), 0)
    assert [ops.resblock_pair_tile_rows(32, K) for K in (3, 7, 11)] == [510, 506, 502]
    assert [ops.resblock3_tile_rows(C) for C in (128, 64, 32)] == [200, 488, 104]
    assert ops.resblock3_tile_rows(32, (1, 2, 4)) == 232
    # refused: C, even K, (K - 1) dil > 64, frag outside C = 64 / 128 and K = 7 / 11, dilations past the halo, null
    assert ops.resblock_pair_tile_rows(48, 3) == 0 and ops.resblock_pair_tile_rows(32, 4) == 0
    assert ops.resblock_pair_tile_rows(32, 11, 7) == 0
    assert ops.resblock_pair_tile_rows(32, 7, 1, frag=True) == 0 and ops.resblock_pair_tile_rows(64, 3, 1, frag=True) == 0
    assert ops.resblock3_tile_rows(16) == 0 and ops.resblock3_tile_rows(32, (1, 3, 9)) == 0
    assert ops.resblock3_tile_rows(64, (4, 4, 4)) == 0
    assert _lib.lib().vo_resblock3_tile_rows(32, None) == 0
