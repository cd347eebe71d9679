"""Checker of one fused ResBlock call (vo_resblock_pair, vo_resblock_pair_frag, vo_resblock3, vo_resblockk) against
float64, per element and per row, with guard utterances around every buffer -- the ResBlock twin of conv_check.

A case is a dict (see ``case``).  ``make`` draws its operands on the CPU and lays them out with guards, ``reference``
computes the float64 result and the element bar, a caller runs the GPU op (or, in the CPU self-test, ``emulate``) on
the views, and ``verify`` checks guards, values and rows.  ``routes`` / ``lengths`` / ``matrix`` name the shipped
dense routes and the lengths every route is run at; tests/test_gpu_resblock_edges.py runs them on the GPU with tile
rows asked of the library, tests/test_resblock_check.py runs ``emulate`` on the same cases with ``FIXED_TILE_ROWS``.

Operands.  x, acc and the weights are bf16 values (rounded before the reference sees them), the biases fp32; b1 and
b2 are drawn with standard deviation 0.5, so that a T1 / x_1 / x_2 row computed from padding (lrelu(b1 + ...)) where
it must be zero is many times over the bar; weights randn / sqrt(C K).

Layout.  x is the contiguous middle of a (B + 2, T, C) buffer whose outer utterances hold conv_check.X_GUARD
(finite, 1e4: a halo row read from there is a gross error, not a NaN that a mask could hide).  y -- and acc where
it aliases y (MRF) -- is the middle of a (B + 2, T, C) buffer whose outer utterances hold the bit pattern
conv_check.Y_GUARD[bf16]; a non-aliased acc sits between X_GUARD utterances like x.

Reference (float64, the computation include/vonoma.h documents), per stage s with x_0 = x:
    a   = lrelu(x_s)                      stage 0: in fp32, rounded to bf16 -- the staged MFMA operand, exactly the
                                          kernel's, as conv_check.staged_input; later stages: float64, unrounded
    t   = lrelu(c1_s(a) + b1_s)           rows outside [0, T) are zero (c2's zero padding)
    x_{s+1} = x_s + c2_s(t) + b2_s        rows outside [0, T) are zero (the next c1's zero padding)
    y   = x_last * out_scale (+ acc)
The on-chip intermediates (T1, x_1, x_2) are NOT rounded in the reference: their rounding is part of the bar.  (A
rounded reference would need a whole bf16 ulp for ties that fall the other way; the unrounded one needs half.)

Element bar: |got - ref| <= e_y, carried through the same pipeline on absolute values.  f = 2^-24 (fp32 unit
roundoff), hu(v) half a bf16 ulp of v's binade, 2^(floor(log2 |v|) - 8) (what storing v as bf16 adds; taken at
|v| + the error v already carries, so a value pushed over a power of two is covered), R = C K,
D(A) = 2 (R + 8) f A the any-order fp32 dot-product bound of conv_check for a sum whose absolute terms add up to A.
    e_{x_0} = 0, and stage 0's a is the reference's own rounding: e_a = 0
    e_a     = e_{x_s} + hu(a)                                     (s > 0: lrelu is 1-Lipschitz; a is staged as bf16)
    e_t     = conv(e_a, |w1|) + D(conv(|a|, |w1|) + |b1|) + hu(t) (lrelu 1-Lipschitz; T1 stored as bf16)
    e_{x_{s+1}} = e_{x_s} + conv(e_t, |w2|) + D(conv(|t|, |w2|) + |b2| + |x_s| [+ |acc / out_scale|])
                  + hu(x_{s+1})           (the last term where x_{s+1} is rounded on chip: not in the last stage)
    e_y     = |out_scale| e_{x_last} + 2 f (|x_last out_scale| + |acc|) + hu(y)
hu(v) lies between 2^-9 |v| and 2^-8 |v|.  The flat u = 2^-9 |v| is the half ulp at the top of a binade only: a
bar built from it is exceeded by round-to-nearest itself (the stand-in, whose arithmetic is the kernels', reaches
1.56 times such a bar), and the flat 2^-8 |v| of conv_check is up to twice what is needed.
The bracketed term is the MRF accumulator of the identity-MFMA path (mrf_acc_mode 2): acc / out_scale with
1 / out_scale a bf16 value is exact in fp32 for bf16 acc and joins the last c2's accumulation; out_scale *
(1 / out_scale) differs from 1 by at most f, which 2 f |acc| covers, as it covers the epilogue add's one rounding.
Rows outside [0, T) carry no error (they are exact zeros on both sides).  Second-order terms are dropped, as
in conv_check.  No term is fitted to a kernel's output.

Row bar: for every (b, t), ||got - ref|| / ||ref|| over the C channels < ROW_TOL = 1e-2 -- the project's bf16 module
tolerance, per row instead of per tensor: the element bar is a worst-case bound and loose for deep reductions.
The CPU stand-in stays at or under STANDIN_ROW_MAX = 5e-3 on every case of the matrix (tests/test_resblock_check.py).

CPU stand-in (``emulate``): the kernels' arithmetic in torch -- fp32 convs on the bf16 operands, T1 / x_1 / x_2
rounded to bf16 and zero outside [0, T), the output rounded to bf16 into the guarded view -- with named mutations,
each a real bug class (``MUTATIONS``).
"""

import numpy as np
import torch
import torch.nn.functional as F

from conv_check import X_GUARD, Y_GUARD

F32 = 2.0 ** -24
ROW_TOL = 1e-2
STANDIN_ROW_MAX = 5e-3
BF16_GUARD = Y_GUARD[torch.bfloat16]
ENTRIES = ("pair", "pair_frag", "block3", "blockk")
ACC_MODES = {"none": 1.0, "mrf": 1.0 / 3, "add": 0.3}  # out_scale; "mrf": acc aliases y, 1 / out_scale a bf16 value
MUTATIONS = ("t1_pad", "x1_pad", "tile_mask", "leak_row", "drop_tap_edge", "zero_group", "stale_halo", "guard",
             "acc_scale")
TILE_LOCAL = ("drop_tap_edge", "zero_group", "stale_halo")  # need ``tile``, the tile's output rows


def case(entry, B, T, C, K, dils, *, slope=0.1, acc="none", knob=None, seed=None, name=None, bias_std=0.5):
    """entry: one of ENTRIES; dils: one dilation (pair entries) or three (whole-block entries); acc: a key of
    ACC_MODES; knob: (key, value) of vo_tune to hold during the call, e.g. ("pair_cfg", 93); bias_std: 0.5, and
    0.1 only where the self-test shows what the earlier draw let through."""
    dils = tuple(int(d) for d in dils)
    assert entry in ENTRIES and acc in ACC_MODES and K % 2 == 1
    assert len(dils) == (1 if entry in ("pair", "pair_frag") else 3)
    c = dict(entry=entry, B=B, T=T, C=C, K=K, dils=dils, slope=slope, acc=acc, knob=knob, bias_std=bias_std,
             out_scale=float(np.float32(ACC_MODES[acc])))
    # the seed does not depend on the accumulator mode: the modes of one shape share operands and reference
    c["seed"] = seed if seed is not None else (B * 1000003 + T * 1009 + C * 31 + K * 7 + sum(dils)) % (2 ** 31)
    c["name"] = name or (f"{entry}_B{B}_T{T}_C{C}_K{K}_d{'-'.join(map(str, dils))}_{acc}" +
                         (f"_{knob[0]}{knob[1]}" if knob else ""))
    return c


def halo(c):
    """Rows of x a row of y depends on, per side: the summed halo of the stages."""
    return sum((d + 1) * (c["K"] - 1) // 2 for d in c["dils"])


def _guarded(val, fill):
    B, T, C = val.shape
    buf = torch.full((B + 2, T, C), fill, dtype=torch.bfloat16)
    buf[1:B + 1] = val
    return buf


def make(c):
    """CPU operands of the case: x / y (/ acc) are the contiguous middles of guarded buffers."""
    g = torch.Generator().manual_seed(c["seed"])
    B, T, C, K = c["B"], c["T"], c["C"], c["K"]
    n = len(c["dils"])
    x = torch.randn(B, T, C, generator=g).bfloat16()
    m = dict(x_val=x.float())
    m["w1"] = [(torch.randn(C, C, K, generator=g) / (C * K) ** 0.5).bfloat16().float() for _ in range(n)]
    m["w2"] = [(torch.randn(C, C, K, generator=g) / (C * K) ** 0.5).bfloat16().float() for _ in range(n)]
    m["b1"] = [torch.randn(C, generator=g) * c["bias_std"] for _ in range(n)]
    m["b2"] = [torch.randn(C, generator=g) * c["bias_std"] for _ in range(n)]
    acc = torch.randn(B, T, C, generator=g).bfloat16()  # drawn last and always: x and the weights do not move
    # [K][Co][Ci] bf16 packs (vo_pack_weight VO_PACK_CONV)
    m["p1"] = [w.permute(2, 0, 1).contiguous().bfloat16() for w in m["w1"]]
    m["p2"] = [w.permute(2, 0, 1).contiguous().bfloat16() for w in m["w2"]]
    m["x_buf"] = _guarded(x, X_GUARD)
    m["x"] = m["x_buf"][1:B + 1]
    ybuf = torch.empty((B + 2, T, C), dtype=torch.bfloat16)
    ybuf.view(torch.int16).fill_(BF16_GUARD)
    m["y_buf"], m["y"] = ybuf, ybuf[1:B + 1]
    m["acc_val"], m["acc_buf"], m["acc"] = None, None, None
    if c["acc"] == "mrf":
        m["y"].copy_(acc)
        m["acc_val"], m["acc"] = acc.float(), m["y"]
    elif c["acc"] == "add":
        m["acc_buf"] = _guarded(acc, X_GUARD)
        m["acc_val"], m["acc"] = acc.float(), m["acc_buf"][1:B + 1]
    m["x_orig"] = m["x_buf"].clone()
    m["acc_orig"] = m["acc_buf"].clone() if m["acc_buf"] is not None else None
    return m


def _half_ulp(v, e=0.0):
    """Half a bf16 ulp (8 significant bits) of the binade of |v| + e: what storing as bf16 a value within e of v can
    add to its error; between 2^-9 and 2^-8 of the magnitude."""
    mag = (v.abs() + e).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(mag)) - 8)


def _lrelu(v, slope):
    return torch.maximum(v, v * slope)


def _conv(x, w, dil):
    """'same' conv of channels-last x (B, T, C) with w (Co, Ci, K), zero padding, in x's dtype."""
    K, T = w.shape[2], x.shape[1]
    h = dil * (K - 1) // 2
    xp, w = F.pad(x, (0, 0, h, h)), w.to(x.dtype)
    return sum(xp[:, k * dil:k * dil + T] @ w[:, :, k].T for k in range(K))  # one GEMM per tap: fast in float64 too


_CORE = {}  # one slot: the accumulator modes of one shape follow each other


def _core(c, m):
    """(x_last, e_{x_last} without the last D term's accumulator part, D's factor) in float64: what the accumulator
    modes of one shape share (the operands are a function of the key's fields alone)."""
    key = (c["seed"], c["B"], c["T"], c["C"], c["K"], c["dils"], c["slope"], c["bias_std"])
    if key not in _CORE:
        _CORE.clear()
        _CORE[key] = _core_compute(m, c["C"], c["K"], c["dils"], c["slope"])
    return _CORE[key]


def _core_compute(m, C, K, dils, slope):
    s32 = torch.tensor(slope, dtype=torch.float32)
    s64 = float(s32)
    dfac = 2 * (C * K + 8) * F32
    x = m["x_val"].double()
    ex = torch.zeros_like(x)
    for s, d in enumerate(dils):
        w1, w2, b1, b2 = m["w1"][s].double(), m["w2"][s].double(), m["b1"][s].double(), m["b2"][s].double()
        if s == 0:
            a = _lrelu(m["x_val"], s32).bfloat16().double()
            ea = ex
        else:
            a = _lrelu(x, s64)
            ea = ex + _half_ulp(a, ex)
        t = _lrelu(_conv(a, w1, d) + b1, s64)
        et = _conv(ea, w1.abs(), d) + dfac * (_conv(a.abs(), w1.abs(), d) + b1.abs())
        et = et + _half_ulp(t, et)
        xn = x + _conv(t, w2, 1) + b2
        ex = ex + _conv(et, w2.abs(), 1) + dfac * (_conv(t.abs(), w2.abs(), 1) + b2.abs() + x.abs())
        if s + 1 < len(dils):
            ex = ex + _half_ulp(xn, ex)
        x = xn
    return x, ex, dfac


def reference(c, m):
    """(ref, bar) in float64 (B, T, C); bar is the element-wise bound of the module docstring."""
    x, ex, dfac = _core(c, m)
    sc = c["out_scale"]
    y = x * sc
    extra = 2 * F32 * y.abs()
    if c["acc"] != "none":
        accv = m["acc_val"].double()
        y = y + accv
        extra = extra + 2 * F32 * accv.abs()
        if c["acc"] == "mrf":
            ex = ex + dfac * (accv / sc).abs()
    bar = abs(sc) * ex + extra
    return y, bar + _half_ulp(y, bar)


def verify(c, m, ref, bar):
    """Guards first (the y buffer's outer utterances bit-identical, the x buffer and a non-aliased acc unchanged),
    then every output finite, the element bar, the row bar.  The AssertionError names which: "guard", "element bar"
    or "row bar".  Returns (worst error / bar, worst row value)."""
    name = c["name"]
    raw = m["y_buf"].view(torch.int16)
    touched = raw[[0, -1]] != BF16_GUARD
    assert not bool(touched.any()), f"{name}: guard: {int(touched.sum())} elements of y's guard utterances written, " \
                                    f"first at {tuple(int(i) for i in touched.nonzero()[0])} (0 = before, 1 = after)"
    assert torch.equal(m["x_buf"].view(torch.int16), m["x_orig"].view(torch.int16)), f"{name}: guard: x buffer changed"
    if m["acc_buf"] is not None:
        assert torch.equal(m["acc_buf"].view(torch.int16), m["acc_orig"].view(torch.int16)), \
            f"{name}: guard: acc buffer changed"
    got = m["y"].double()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    rows = (got - ref).norm(dim=2) / ref.norm(dim=2).clamp_min(1e-30)
    rowmax = float(rows.max())
    print(f"{name}: worst error/bar {ratio:.3e}, worst row {rowmax:.3e}")
    over = err > bar
    assert not bool(over.any()), f"{name}: element bar: {int(over.sum())} of {over.numel()} elements over " \
                                 f"(worst ratio {ratio:.3g}), first at {tuple(int(i) for i in over.nonzero()[0])}"
    bad = rows >= ROW_TOL
    assert not bool(bad.any()), f"{name}: row bar: {int(bad.sum())} of {bad.numel()} rows at or over {ROW_TOL} " \
                                f"(worst {rowmax:.3g}), first at {tuple(int(i) for i in bad.nonzero()[0])}"
    return ratio, rowmax


def emulate(c, m, mutate=None, tile=None):
    """The CPU stand-in for the kernels: their arithmetic in fp32 torch on the operands as laid out in memory,
    written into the y view.  Every utterance is computed on a frame of halo(c) extra rows per side whose rows
    outside [0, T) are zero in x, T1, x_1 and x_2 -- the masks the mutations remove.  ``mutate`` names a deliberate
    fault (MUTATIONS); ``tile`` is the tile's output rows for the faults local to a tile (TILE_LOCAL)."""
    assert mutate is None or mutate in MUTATIONS
    assert mutate not in TILE_LOCAL or tile
    B, T, C, K, dils = c["B"], c["T"], c["C"], c["K"], c["dils"]
    H, h2 = halo(c), (K - 1) // 2
    slope = torch.tensor(c["slope"], dtype=torch.float32)
    sc = torch.tensor(c["out_scale"], dtype=torch.float32)
    inside = torch.zeros(B, T + 2 * H, 1, dtype=torch.bool)
    inside[:, H:H + T] = True
    masked = inside.clone()  # where T1 is masked to zero outside [0, T)
    if mutate == "t1_pad":
        masked[:] = True
    if mutate == "tile_mask":  # only the batch's first and last tile know they are boundary tiles
        masked[:] = True
        masked[0, :H] = False
        masked[-1, H + T:] = False
    xs = F.pad(m["x"].float(), (0, 0, H, H))
    if mutate == "leak_row":  # utterance b > 0: the row before its first is the last row of utterance b - 1
        xs[1:, H - 1] = m["x"][:-1, T - 1].float()
    rows = torch.arange(T)
    for s, d in enumerate(dils):
        last = s + 1 == len(dils)
        w1, w2 = m["p1"][s].float().permute(1, 2, 0), m["p2"][s].float().permute(1, 2, 0)
        a = _lrelu(xs, slope).bfloat16().float()
        t = _lrelu(_conv(a, w1, d) + m["b1"][s], slope).bfloat16().float() * masked
        v = _conv(t, w2, 1)
        if last and mutate == "drop_tap_edge":  # c2's last tap (it reads T1 row r + h2) in each tile's last row
            r = rows[(rows % tile) == tile - 1]
            v[:, H + r] -= torch.einsum("oi,bri->bro", w2[:, :, K - 1], t[:, H + r + h2])
        if last and mutate == "stale_halo":  # the tile's first h2 rows from T1 one tile of rows earlier
            r = rows[(rows >= tile) & (rows % tile < h2)]
            v[:, H + r] = _conv(torch.roll(t, tile, dims=1), w2, 1)[:, H + r]
        v = v + m["b2"][s] + xs
        if not last:
            xs = v.bfloat16().float()
            if mutate != "x1_pad":
                xs = xs * inside
    v = v[:, H:H + T]
    if c["acc"] == "none":
        y = v * sc
    elif mutate == "acc_scale":
        y = (v + m["acc"].float()) * sc
    elif c["acc"] == "mrf":  # the identity-MFMA path: acc / out_scale joins the accumulator
        y = (v + m["acc"].float() * (1.0 / sc)) * sc
    else:
        y = v * sc + m["acc"].float()
    if mutate == "zero_group":  # one 8-channel group of the first tile's last row, in the middle utterance
        y = y.clone()
        y[B // 2, min(tile, T) - 1, C - 8:] = 0
    m["y"].copy_(y.bfloat16())
    if mutate == "guard":
        m["y_buf"].view(torch.int16)[-1, 0, 0] += 1


# ---------------------------------------------------------------- the shipped dense routes and their lengths
# name -> (entry, C, K, [dils, ...], knob, accumulator modes).  Pairs: dilation 1 and the largest the vocoder uses (5).
# blockk has no epilogue-add mode (VO_NOT_HANDLED by contract).
_ALL = ("none", "mrf", "add")
_D135 = (1, 3, 5)


def routes():
    r = {}
    for C, K in [(32, 3), (32, 7), (32, 11), (64, 3), (64, 5), (64, 9), (64, 7), (64, 11), (128, 3), (128, 5),
                 (128, 9), (128, 7), (128, 11)]:
        r[f"pair_C{C}_K{K}"] = ("pair", C, K, [(1,), (5,)], None, _ALL)
    for C in (64, 128):
        for K in (7, 11):
            r[f"pair_C{C}_K{K}_cfg93"] = ("pair", C, K, [(1,), (5,)], ("pair_cfg", 93), _ALL)  # LDS-tile kernels
            r[f"frag_C{C}_K{K}"] = ("pair_frag", C, K, [(1,), (5,)], None, _ALL)
    r["block3_C64"] = ("block3", 64, 3, [_D135], None, _ALL)     # planes
    r["block3_C128"] = ("block3", 128, 3, [_D135], None, _ALL)   # planes
    r["block3_C32"] = ("block3", 32, 3, [_D135], None, _ALL)     # register frames
    r["block3_C32_d124"] = ("block3", 32, 3, [(1, 2, 4)], None, _ALL)                    # LDS frames, no knob
    r["block3_C32_cfg80"] = ("block3", 32, 3, [_D135], ("rb3_cfg", 80), _ALL)            # LDS frames
    r["blockk_K7"] = ("blockk", 32, 7, [_D135], None, ("none", "mrf"))
    r["blockk_K11"] = ("blockk", 32, 11, [_D135], None, ("none", "mrf"))
    return r


# The tile rows of today's shipped library per route and dilation(s), for the CPU self-test alone (no library
# call on that path); the GPU test asks the library, and tests/test_resblock_check.py compares the two when the
# library is built.
def _fixed_tile_rows():
    t = {}
    for name, (entry, C, K, _, knob, _) in routes().items():
        if entry in ("pair", "pair_frag"):
            r1 = 512 if C == 32 else (256 if (C == 128 or K == 3) else 512)
            t[name] = r1 - (K - 1)
    t.update(block3_C64=488, block3_C128=200, block3_C32=104, block3_C32_d124=232, block3_C32_cfg80=232,
             blockk_K7=952, blockk_K11=904)
    return t


FIXED_TILE_ROWS = _fixed_tile_rows()


# (entry, T, C, K, dils) -> seed, for the cases whose default draw put the stand-in's worst row value over
# STANDIN_ROW_MAX (block3 T = 231 (1, 2, 4): 5.4e-3; blockk T = 951 / 953 / 1907 at K = 7 and 903 at K = 11: 5.0e-3 to
# 5.6e-3) or within 3 % of it.  At C = 32 with three stages the worst of a few thousand rows lies near 5e-3 for many
# draws; these seeds give 4.1e-3 to 4.6e-3.  The bars are the same for every seed.
SEEDS = {
    ("block3", 104, 32, 3, (1, 3, 5)): 12, ("block3", 211, 32, 3, (1, 3, 5)): 31, ("block3", 231, 32, 3, (1, 2, 4)): 16,
    ("block3", 232, 32, 3, (1, 3, 5)): 24, ("block3", 467, 32, 3, (1, 3, 5)): 28,
    ("blockk", 951, 32, 7, (1, 3, 5)): 27, ("blockk", 952, 32, 7, (1, 3, 5)): 36, ("blockk", 953, 32, 7, (1, 3, 5)): 8,
    ("blockk", 1907, 32, 7, (1, 3, 5)): 8, ("blockk", 903, 32, 11, (1, 3, 5)): 38, ("blockk", 904, 32, 11, (1, 3, 5)): 30,
}


def lengths(entry, K, dils):
    """{id: bt -> T}: 1, h, h + 1, BT - 1, BT, BT + 1, 2 BT + 3 (h = (K - 1) / 2; at K = 3 h is the 1 already there)
    and, for the whole-block entries, the summed halo of the three stages -+ 1."""
    h = (K - 1) // 2
    ts = {"T1": lambda bt: 1, "h": lambda bt: h, "h+1": lambda bt: h + 1, "BT-1": lambda bt: bt - 1,
          "BT": lambda bt: bt, "BT+1": lambda bt: bt + 1, "2BT+3": lambda bt: 2 * bt + 3}
    if h == 1:
        del ts["h"]
    if entry in ("block3", "blockk"):
        hl = sum((d + 1) * h for d in dils)
        ts.update({"halo-1": lambda bt: hl - 1, "halo+1": lambda bt: hl + 1})
    return ts


def matrix_ids():
    """[(route, dils, length id, accumulator mode)]: the GPU test's parameters, independent of the tile rows."""
    return [(name, tuple(dils), lid, acc) for name, (entry, C, K, dil_list, _, accs) in routes().items()
            for dils in dil_list for lid in lengths(entry, K, dils) for acc in accs]


def matrix_case(name, dils, lid, acc, bt):
    """The case of one matrix_ids() entry for a route whose tile has bt output rows; B = 3."""
    entry, C, K, _, knob, _ = routes()[name]
    T = lengths(entry, K, dils)[lid](bt)
    return case(entry, 3, T, C, K, dils, acc=acc, knob=knob, seed=SEEDS.get((entry, T, C, K, tuple(dils))))


def matrix(tile_rows):
    """Every case of the GPU test: [(route, tile rows, case)].  tile_rows(route name, entry, C, K, dils, knob) -> the
    route's output rows per tile."""
    out = []
    for name, dils, lid, acc in matrix_ids():
        entry, C, K, _, knob, _ = routes()[name]
        bt = tile_rows(name, entry, C, K, dils, knob)
        assert bt > 0, name
        out.append((name, bt, matrix_case(name, dils, lid, acc, bt)))
    return out
