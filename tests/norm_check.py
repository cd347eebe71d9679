"""Checker of one LayerNorm or BatchNorm call (csrc/layernorm.hip, csrc/batchnorm.hip)
against float64, element by element, with guard bands around every buffer.

A case is a dict (``ln_case`` / ``bn_case``).  ``make`` draws its operands on the CPU (bf16-exact where the
kernel reads bf16) and lays every tensor inside a larger flat buffer: outputs between conv_check.Y_GUARD's
fixed bit patterns, inputs between finite sentinels (1e4).  ``reference`` is the closed form in float64 with its
bars, a runner (the GPU test, or ``standin`` in the CPU self-test) fills the outputs, ``verify`` checks, in
this order and naming the first that fails: guard, operand, pad row, non-finite, copy, element bar, rel-L2.

LayerNorm (u = 2^-24, D the row length, per row).  The kernels form v = fl32(fl32(drop(x) scale) + res) and the
reference starts from that fp32 v, so everything below is the error of fp32 arithmetic on v:
  * mean: a sum of D terms in any order, |dmean| <= D u (|mean| + max|v - mean|) =: D u A.  Relative to the
    row's spread that is cond = D u A rstd -- the condition term: it is all that grows when a row's mean
    dwarfs its spread.  The two-pass variance about a mean that is off by dmean is var + dmean^2 exactly, so
    rstd is off by er = (D + 16) u + cond^2 relative (the any-order sum of D squares, the rounding of each
    difference and square, rsqrt to a few ulp; cond^2 >= dmean^2 / (var + eps) / 2).
  * xhat = (v - mean) rstd:  ex = cond + |xhat| er.
  * y = xhat gamma + beta:   |gamma| ex + 2 u (|gamma xhat| + |beta|)   [+ 2^-8 |ref| for a bf16 y: half an ulp of
    bf16 is at most 2^-8 of the value; precisely 2^-8 (|ref| + bar), the rounded value being within bar of ref].
  * backward, gd = gamma dy (dy = fl32(gy + gy2) as the kernel adds them), m1 = mean(gd), m2 = mean(gd xhat),
    gh = rstd (gd - m1 - xhat m2):  with em1 = (D + 2) u mean|gd|, em2 = (D + 2) u mean|gd xhat| + mean(|gd| ex),
    bar = rstd ((er + 4 u) (|gd| + mean|gd| + |xhat| mean|gd xhat|) + em1 + ex mean|gd xhat| + |xhat| em2);
    through the dropout the x gradient is that times scale (+ u), gres is it as it stands; bf16: + 2^-8 |ref|.
  * dgamma = sum over live rows of dy xhat, dbeta of dy: the any-order fp32 sum bound of wgrad_check.py,
    2 (R + 8) u sum|term| with R the live rows, plus for dgamma sum(|dy| ex).
    One row left out moves an element by about one term, 2^23 / R^2 bars: ``applies`` offers ``drop_partial``
    only to cases with R <= R_MAX live rows.
Pad rows (t >= lens[b]) of every LayerNorm output must be exactly zero.  The inputs of pad rows hold NaN: the
forward never reads them, the backward reads row 0 in a dead row's place and must drop it by selection
(``lens[0] == 0`` makes row 0 itself such a row).  y16 must be bf16(y) bit for bit.

BatchNorm (per channel, M rows).  depth = the number of Welford steps / merges a value passes on its way into
the channel's triple, from the route record: ceil(min(RB, rows) / RL) in its lane, RL (FLAT: V + 8) lane merges,
ceil(nb / 8) + 8 block merges (scalar route: nb).  A step rounds the new mean once (u |mean|) and its small
    increment twice; the sums of squares round a handful of times per step: k = 4 depth.
  * mean: the bar of an fp32 mean of M terms taken depth at a time, bm = 2 depth u A, A = |mean| + 2 max|x - mean|
    (the 2: the vectorised kernels sum x - x_first, and |x - x_first| <= 2 max|x - mean|).
  * var: ev = k u (var + 2 max|x - mean|^2) + 4 max|x - mean| bm (the sums of squares about a shift that is a
    data value; the merges' (mean_b - mean_a)^2 with both means off by bm), rstd relative: er = ev / (var + eps) / 2
    + 4 u -- ev / (var + eps) is the variance's condition number times the rounding.
  * y = (x - mean) rstd gamma + beta: |gamma| (bm rstd + |xhat| er) + 3 u (|gamma xhat| + |beta|) [+ 2^-8 |ref|].
  * running: (1 - m) r + m stat, the variance unbiased (M / (M - 1); M = 1: the biased one, the kernels'
    documented ``unb = var``): m bm + 3 u (|r| + |mean|), m ev M / (M - 1) + 3 u (|r| + |unb|).
  * backward (mean_rstd is an input: the fp32 values the forward left): xhat = (x - mu) rs to 3 u,
    dbeta = sum dy, dgamma = sum dy xhat: 2 (M + 8) u sum|term| (+ 3 u sum|dy xhat|);
    dx = gamma rs (dy - dbeta / M - xhat dgamma / M) from the kernel's own sums:
    |gamma rs| (6 u (|dy| + |dbeta| / M + |xhat dgamma| / M) + bar(dbeta) / M + |xhat| bar(dgamma) / M).
    FLAT backward: the kernel works in double and rounds once, so dx, dgamma and dbeta get half an ulp of the
    output format, 2^-24 |ref| (bf16 dx: 2^-8 |ref|), plus 2^-48 of the magnitudes for the double arithmetic.
Whole tensor: rel-L2 < 1e-5 (the project's fp32 tolerance) on fp32 outputs of well-conditioned cases (profiles
plain / tiny / first_outlier), 2^-8 on bf16 ones (half an ulp is 2^-9 per element).  Ill-conditioned profiles
(offset, constant): 4 x the rel-L2 the fp32 stand-in reaches on the same operands, measured by the CPU
self-test and written beside the case (``ill`` of the case; the factor 4 is the mel front end's).
"""

import math

import torch

from conv_check import X_GUARD, Y_GUARD

U = 2.0 ** -24
EPS = 1e-5
GUARD_N = 64            # guard elements on each side of every tensor
WS_GUARD_N = 256
R_MAX = 1200
REL_L2_F32, REL_L2_BF16, OLD_BF16_REL_L2 = 1e-5, 2.0 ** -8, 1e-2
ILL = ("offset", "constant")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64}
BN_FIELDS = ("route", "V", "CV", "RL", "RB", "nb", "apply_blocks", "CT")
SCALAR, VEC, FLAT = 0, 1, 2
LN_ENTRIES = ("fwd", "dual", "drop", "bwd", "bwd_ex", "bwd_drop")
FAILURES = ("guard", "operand", "pad row", "non-finite", "copy", "num_batches", "element bar", "rel-L2")
# name -> the failure verify must name (a regular expression).  A one-pass variance at C = 1 is off by 2 % on a
# channel whose mean is 10^3 spreads: less than the worst case of the Welford merges there, which is why the
# ill-conditioned cases also carry the whole-tensor bar of 4 x the stand-in's rel-L2
MUTATIONS = {
    "one_pass_var": "(element bar|rel-L2)", "biased_running_var": "element bar", "pad_row_live": "pad row",
    "drop_partial": "element bar", "row_shift": "element bar", "mask_off_by_one": "pad row",
    "no_gy2": "element bar", "drop_unscaled": "element bar", "write_past": "guard",
    "shift_first_outlier": "(element bar|rel-L2)"}


# ---------------------------------------------------------------------------------------------- cases

def lens_of(c):
    """The per-utterance lengths of a LayerNorm case (None: no lens tensor)."""
    B, T, spec = c["B"], c["T"], c["lens"]
    if spec is None:
        return None
    if isinstance(spec, (list, tuple)):  # the lengths themselves
        assert len(spec) == B and all(0 <= n <= T for n in spec), spec
        return list(spec)
    if spec == "full":
        return [T] * B
    if spec == "one":
        return [1] * B
    if spec == "zero_mid":
        return [0 if b == B // 2 else T for b in range(B)]
    if spec == "zero_first":
        return [0] + [max(1, T - 1 - b % 3) for b in range(1, B)]
    assert spec == "mixed", spec
    return [T if b == B - 1 else min(T, (3, 0, 2, 5, 1)[b % 5]) for b in range(B)]


def ln_case(entry, B, T, D, tx, tr, t3, *, res=True, p=None, gy2=False, gres=None, y16=False, lens=None,
            profile="plain", ill=None):
    """One LayerNorm call.  entry: LN_ENTRIES; tx / tr: dtypes of x and res; t3: of y (forward) or gy (backward).
    res False: no residual (vo_layernorm, vo_layernorm_bwd).  p: the dropout rate of the drop entries.  gy2: the
    bf16 gradient of the y16 copy.  gres: the separate residual gradient (bwd_ex's gh32, bwd_drop's gres).  y16:
    the drop forward's bf16 copy.
    ill: {output: rel-L2 of the fp32 stand-in} for the ill-conditioned profiles."""
    assert entry in LN_ENTRIES and D in (256, 512)
    bwd = entry.startswith("bwd")
    drop = entry in ("drop", "bwd_drop")
    assert (p is not None) == drop
    dual = entry == "dual" or (entry == "drop" and y16)
    if gres is None or not bwd:
        gres = entry in ("bwd_ex", "bwd_drop") if bwd else False
    c = dict(kind="ln", entry=entry, B=B, T=T, D=D, tx=tx, tr=tr if res else tx, t3=t3, res=bool(res), p=p,
             gy2=bool(gy2), gres=bool(gres), dual=bool(dual), lens=lens, profile=profile, bwd=bwd, drop=drop,
             ill=ill)
    c["name"] = (f"ln_{entry}_{tx}_{c['tr']}_{t3}_D{D}_B{B}_T{T}" + ("" if res else "_nores") +
                 (f"_p{p}" if drop else "") + ("_gy2" if gy2 else "") + ("_y16" if dual and entry == "drop" else "") +
                 ("_nogres" if entry == "bwd_ex" and not gres else "") +
                 (f"_{lens}" if lens else "") + ("" if profile == "plain" else f"_{profile}"))
    c["seed"] = (B * 1000003 + T * 1009 + D * 31 + len(c["name"]) * 7) % (2 ** 31)
    c["salt"] = 1 + c["seed"] % 97
    return c


def seed_value(c):
    """The int64 dropout seed of a drop case (the mask is vo_dropout's for this seed and c["salt"])."""
    return c["seed"] * 2654435761 % (2 ** 62)


def ln_nblk(c):
    return (c["B"] * c["T"] + 63) // 64


def bn_case(M, C, tx, tg=None, *, affine=True, running=True, profile="plain", misaligned=False, rec_fwd=None,
            rec_bwd=None, ill=None):
    """One BatchNorm forward and one backward on the same x.  tg: dtype of dy (None: x's).  misaligned: x, dy and
    the outputs start 60 bytes (fp32) / 30 elements (bf16) into a 16-byte line.  rec_fwd / rec_bwd: the
    vo_bn_route records the two calls must get (BN_FIELDS order)."""
    tg = tg or tx
    c = dict(kind="bn", M=M, C=C, tx=tx, tg=tg, affine=bool(affine), running=bool(running), profile=profile,
             misaligned=bool(misaligned), rec_fwd=rec_fwd, rec_bwd=rec_bwd, ill=ill, eps=EPS, momentum=0.1)
    c["name"] = (f"bn_{tx}_{tg}_M{M}_C{C}" + ("" if affine else "_noaffine") + ("" if running else "_norun") +
                 ("_misaligned" if misaligned else "") + ("" if profile == "plain" else f"_{profile}"))
    c["seed"] = (M * 1000003 + C * 1009 + len(c["name"]) * 7) % (2 ** 31)
    return c


def record(c, which):
    return dict(zip(BN_FIELDS, c["rec_" + which]))


def route_args(c, which, ptrs=None):
    """Arguments of ops.bn_route for the forward / backward of a case; ptrs: {x, dy, y, dx} addresses (None: the
    case's declared alignment on made-up addresses)."""
    if ptrs is None:
        off = 60 if c["misaligned"] else 0
        ptrs = dict(x=4096 + off, dy=8192 + off, y=12288 + off, dx=16384 + off)
    if which == "fwd":
        return (c["M"], c["C"], TDT[c["tx"]], None, ptrs["x"], None, ptrs["y"])
    return (c["M"], c["C"], TDT[c["tx"]], TDT[c["tg"]], ptrs["x"], ptrs["dy"], ptrs["dx"])


def reached(c):
    """The kernel instantiations and edges a case exercises: LayerNorm (kernel, TX, TR, TY / TG, NPL, DUAL, drop,
    gy2, gres) and the call itself, ("ln_call", entry) + its LN_ACCEPTS form; BatchNorm (kernel, template
    arguments...) from the declared records; edges as strings."""
    out = set()
    if c["kind"] == "ln":
        out.add(("ln_call", c["entry"], c["tx"], c["tr"], c["t3"], c["gy2"] if c["bwd"] else c["dual"],
                 c["bwd"] and c["gres"]))
        npl = c["D"] // 64
        rows = c["B"] * c["T"]
        if c["bwd"]:
            out.add(("layernorm_bwd_kernel", c["tx"], c["tr"], c["t3"], npl, False, c["drop"], c["gy2"], c["gres"]))
            out.add(f"ln_bwd/nblk/{ln_nblk(c)}")
            if rows % 64 == 1:
                out.add("ln_bwd/last_block_one_row")
            if c["lens"] == "zero_first":
                out.add("ln_bwd/row0_is_pad")
        else:
            out.add(("layernorm_kernel", c["tx"], c["tr"], c["t3"], npl, c["dual"], c["drop"], False, False))
            if not c["res"]:
                out.add(("layernorm_kernel/nores", c["tx"], c["t3"], npl))
            out.add("ln_fwd/rows%4==1" if rows % 4 == 1 and rows > 1 else "ln_fwd/one_row" if rows == 1 else "ln_fwd")
        out.add(f"ln/lens/{c['lens']}")
        out.add(f"ln/profile/{c['profile']}")
        if c["drop"]:
            out.add(f"ln/p/{c['p']}")
        return out
    tx, tg = c["tx"], c["tg"]
    for which in ("fwd", "bwd"):
        r = record(c, which)
        fl = r["route"] == FLAT
        if r["route"] == SCALAR:
            if which == "fwd":
                out |= {("bn_stats_kernel", tx, r["CT"]), ("bn_finalize_kernel",), ("bn_apply_kernel", tx)}
            else:
                out |= {("bn_bwd_stats_kernel", tx, tg, r["CT"]), ("bn_bwd_finalize_kernel",),
                        ("bn_bwd_apply_kernel", tx, tg)}
            if c["C"] % 64 == 1 and c["C"] > 1:
                out.add("bn_scalar/one_channel_tile")
            if c["C"] in (2056, 1028):
                out.add(f"bn_scalar/past_vector_limit/{tx}")
            if c["misaligned"]:
                out.add(f"bn_misaligned/{'flat' if c['C'] == 1 else 'vec'}/{which}")
            if which == "bwd" and record(c, "fwd")["route"] != SCALAR and not c["misaligned"]:
                out.add("bn_bwd/bf16_x_f32_dy_falls_back")
        else:
            if which == "fwd":
                out |= {("bn_stats_v_kernel", tx, fl), ("bn_finalize_v_kernel",), ("bn_apply_v_kernel", tx, fl)}
            else:
                out |= {("bn_bwd_stats_v_kernel", tx, tg, fl), ("bn_bwd_apply_v_kernel", tx, tg, fl),
                        ("bn_bwd_finalize_flat_kernel",) if fl else ("bn_bwd_finalize_v_kernel",)}
            if not fl:
                out.add(f"bn_vec/nb/{r['nb']}")
                out.add(f"bn_vec/CV/{r['CV']}")
                if 256 % r["CV"]:
                    out.add(f"bn_vec/idle_threads/{256 - r['RL'] * r['CV']}")
                if (c["M"] - 1) % r["RB"] == 0 and c["M"] > 1:
                    out.add("bn_vec/last_block_one_row")
            else:
                out.add(f"bn_flat/nb/{r['nb']}")
                if c["M"] == r["V"]:
                    out.add(f"bn_flat/one_vector/{tx}")
    out.add(f"bn/profile/{c['profile']}")
    if c["M"] == 1:
        out.add("bn/M1")
    if not c["affine"]:
        out.add("bn/no_affine")
    if not c["running"]:
        out.add("bn/no_running")
    return out


# ---------------------------------------------------------------------------------------------- accept tables

_F, _H = "f32", "bf16"
# entry -> the calls it takes, as (tx, tr, t3, aux, gres): the dtypes of x and res, of y (forward) or gy (backward);
# aux: a y16 (forward) / a gy2 (backward) is passed; gres: the separate residual gradient is passed (bwd_ex's gh32,
# bwd_drop's gres).  Arguments an entry does not have are held at what it implies: vo_layernorm has no y16,
# vo_layernorm_dual an fp32 y and always a y16, vo_layernorm_bwd res of x's dtype, vo_layernorm_bwd_drop always a
# gres.  Everything else ``ln_domain`` lists must be refused (the tables of csrc/layernorm.hip).
LN_ACCEPTS = {
    "fwd": {(_H, _H, _H, False, False), (_F, _F, _F, False, False), (_H, _H, _F, False, False),
            (_F, _F, _H, False, False)},
    "dual": {(_F, _F, _F, True, False), (_H, _H, _F, True, False), (_H, _F, _F, True, False)},
    "drop": {(_H, _H, _H, False, False), (_F, _F, _F, False, False), (_H, _F, _F, False, False),
             (_F, _F, _F, True, False), (_H, _F, _F, True, False)},
    "bwd": {(_H, _H, _H, False, False), (_H, _H, _F, False, False), (_F, _F, _F, False, False),
            (_F, _F, _H, False, False)},
    # res of x's dtype: only without gy2 and gh32 (what vo_layernorm_bwd takes); bf16 x with fp32 res: any
    "bwd_ex": {(_H, _H, _H, False, False), (_H, _H, _F, False, False), (_F, _F, _F, False, False),
               (_F, _F, _H, False, False)} |
              {(_H, _F, tg, gy2, gh32) for tg in (_F, _H) for gy2 in (False, True) for gh32 in (False, True)},
    # res of x's dtype: only without gy2
    "bwd_drop": {(_H, _H, _H, False, True), (_F, _F, _F, False, True)} |
                {(_H, _F, tg, gy2, True) for tg in (_F, _H) for gy2 in (False, True)},
}


def ln_domain(entry):
    """Every call of an entry over {f32, bf16} for each dtype argument it has, with and without each optional
    pointer it has, in the form of LN_ACCEPTS."""
    dts, tf = (_F, _H), (False, True)
    if entry == "fwd":
        return [(tx, tr, ty, False, False) for tx in dts for tr in dts for ty in dts]
    if entry == "dual":
        return [(tx, tr, _F, True, False) for tx in dts for tr in dts]
    if entry == "drop":
        return [(tx, tr, ty, y16, False) for tx in dts for tr in dts for ty in dts for y16 in tf]
    if entry == "bwd":
        return [(tx, tx, tg, False, False) for tx in dts for tg in dts]
    if entry == "bwd_ex":
        return [(tx, tr, tg, gy2, gh32) for tx in dts for tr in dts for tg in dts for gy2 in tf for gh32 in tf]
    assert entry == "bwd_drop", entry
    return [(tx, tr, tg, gy2, True) for tx in dts for tr in dts for tg in dts for gy2 in tf]


def ln_instantiation(entry, combo):
    """The kernel template arguments an accepted call launches, less NPL: forward (TX, TR, TY, DUAL), backward
    (TX, TR, TG)."""
    tx, tr, t3, aux, _ = combo
    return ("layernorm_bwd_kernel", tx, tr, t3) if entry.startswith("bwd") else ("layernorm_kernel", tx, tr, t3, aux)


# ---------------------------------------------------------------------------------------------- buffers

def _bits(t):
    return t.view(_INT[t.dtype])


def _add(m, name, value, kind, lead=0):
    """Lay ``value`` into a flat guarded buffer.  kind: "in" (sentinels 1e4, must stay bit-identical), "out"
    (the guard pattern everywhere), "inout" (the pattern around the values; running statistics), "ws" (NaN
    inside, the pattern after).  lead: extra elements before the tensor (a misaligned start)."""
    dt = value.dtype
    lo = GUARD_N + lead
    n = value.numel()
    hi = WS_GUARD_N if kind == "ws" else GUARD_N
    buf = torch.empty(lo + n + hi, dtype=dt)
    if kind == "in":
        buf.fill_(X_GUARD if dt.is_floating_point else 12345)
    elif dt in Y_GUARD:
        _bits(buf).fill_(Y_GUARD[dt])
    else:
        buf.fill_(0x5A5AA5A5)
    if kind == "out":
        pass
    elif kind == "ws":
        buf[lo:lo + n] = float("nan")
    else:
        buf[lo:lo + n] = value.reshape(-1)
    m["bufs"][name] = buf
    m["spec"][name] = (lo, tuple(value.shape), kind)
    if kind != "ws":
        m["orig"][name] = buf.clone()


def view(m, name, bufs=None):
    """The tensor ``name`` inside its guarded buffer (``bufs``: another set of the same layout, e.g. on the GPU)."""
    lo, shape, _ = m["spec"][name]
    n = math.prod(shape)
    return (bufs or m["bufs"])[name][lo:lo + n].view(shape)


def fresh(m):
    """The same case with every buffer as ``make`` left it (after a run that wrote outputs)."""
    out = dict(m)
    out["bufs"] = {k: (m["orig"][k].clone() if k in m["orig"] else v.clone()) for k, v in m["bufs"].items()}
    for k, (lo, shape, kind) in m["spec"].items():
        if kind == "ws":
            b = out["bufs"][k]
            _bits(b).fill_(Y_GUARD[torch.float32])
            b[lo:lo + math.prod(shape)] = float("nan")
    return out


def _exact(t, dt):
    return t.bfloat16().float() if dt == "bf16" else t.float()


def _profile_rows(c, g, rows, D, dt, role):
    """fp32 values (rows, D) of a LayerNorm operand under the case's profile.  role: "x" or "res"."""
    v = torch.randn(rows, D, generator=g)
    prof = c["profile"]
    if prof == "tiny":
        v = v * 1e-4 if role == "x" else torch.zeros_like(v)
    elif prof == "offset":
        # the offset rides on the fp32 operand where there is one (10^3 row stds); bf16 keeps a spread up to 128:
        # its spacing at 128 is one std
        carrier = "res" if (c["res"] and c["tr"] == "f32") else "x"
        if role == carrier:
            ratio = 1e3 if dt == "f32" else 128.0
            v = v + ratio * (2 * torch.rand(rows, 1, generator=g) - 1)
    elif prof == "constant":
        const = torch.arange(rows) % 3 == 1
        v[const] = (3 * torch.randn(rows, 1, generator=g))[const].expand(-1, D)
    return _exact(v, dt)


def make(c, mask=None):
    """CPU buffers of a case: m["bufs"][name] flat guarded buffers, m["spec"], m["orig"] (inputs and in-out
    tensors as made).  mask (drop entries): the keep mask (B, T, D) bool -- vo_dropout's on the GPU, any on the CPU."""
    g = torch.Generator().manual_seed(c["seed"])
    m = dict(bufs={}, spec={}, orig={})
    if c["kind"] == "ln":
        B, T, D = c["B"], c["T"], c["D"]
        rows = B * T
        x = _profile_rows(c, g, rows, D, c["tx"], "x")
        res = _profile_rows(c, g, rows, D, c["tr"], "res") if c["res"] else None
        gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
        beta = 0.1 * torch.randn(D, generator=g)
        lens = lens_of(c)
        live = torch.ones(B, T, dtype=torch.bool) if lens is None else \
            torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        m["live"] = live.reshape(rows)
        dead = ~m["live"]
        nan = float("nan")
        x[dead] = nan
        _add(m, "x", x.to(TDT[c["tx"]]), "in")
        if res is not None:
            res[dead] = nan
            _add(m, "res", res.to(TDT[c["tr"]]), "in")
        _add(m, "gamma", gamma, "in")
        if lens is not None:
            _add(m, "lens", torch.tensor(lens, dtype=torch.int32), "in")
        if c["drop"]:
            if mask is None:
                mask = torch.rand(rows, D, generator=g) >= c["p"]
            m["mask"] = mask.reshape(rows, D).cpu()
            _add(m, "seed", torch.tensor([seed_value(c)], dtype=torch.int64), "in")
        if not c["bwd"]:
            _add(m, "beta", beta, "in")
            _add(m, "y", torch.empty(rows, D, dtype=TDT[c["t3"]]), "out")
            if c["dual"]:
                _add(m, "y16", torch.empty(rows, D, dtype=torch.bfloat16), "out")
        else:
            gy = _exact(torch.randn(rows, D, generator=g), c["t3"])
            gy[dead] = nan
            _add(m, "gy", gy.to(TDT[c["t3"]]), "in")
            if c["gy2"]:
                gy2 = _exact(torch.randn(rows, D, generator=g), "bf16")
                gy2[dead] = nan
                _add(m, "gy2", gy2.bfloat16(), "in")
            _add(m, "gh", torch.empty(rows, D, dtype=TDT[c["tx"]]), "out")
            if c["gres"]:
                _add(m, "gres", torch.empty(rows, D, dtype=TDT[c["tr"]]), "out")
            _add(m, "dgamma", torch.empty(D), "out")
            _add(m, "dbeta", torch.empty(D), "out")
            _add(m, "ws", torch.empty(ln_nblk(c) * 2 * D), "ws")
        return m
    M, C = c["M"], c["C"]
    r = record(c, "fwd")
    prof = c["profile"]
    std = 1.7
    x = 0.4 + std * torch.randn(M, C, generator=g)
    big = 1e3 if c["tx"] == "f32" else 128.0
    if prof == "offset":
        x = x + big * std * (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.arange(C) % 2))
    elif prof == "constant":
        x[:, 0] = 0.75
    elif prof == "first_outlier":  # the first value of every lane of every block: the vectorised kernels' shift
        first = (torch.arange(M) % r["RB"]) < r["RL"]
        x[first] += big * std
    x = _exact(x, c["tx"])
    dy = _exact(torch.randn(M, C, generator=g), c["tg"])
    lead = {"f32": 15, "bf16": 30}
    lx = lead[c["tx"]] if c["misaligned"] else 0
    lg = lead[c["tg"]] if c["misaligned"] else 0
    _add(m, "x", x.to(TDT[c["tx"]]), "in", lx)
    _add(m, "dy", dy.to(TDT[c["tg"]]), "in", lg)
    if c["affine"]:
        _add(m, "gamma", 1.0 + 0.2 * torch.randn(C, generator=g), "in")
        _add(m, "beta", 0.1 * torch.randn(C, generator=g), "in")
    if c["running"]:
        _add(m, "run_mean", 0.1 * torch.randn(C, generator=g), "inout")
        _add(m, "run_var", 1.0 + 0.1 * torch.rand(C, generator=g), "inout")
        _add(m, "nbt", torch.tensor([7], dtype=torch.int64), "inout")
    x64 = x.double()
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    mr = torch.cat([mean, (var + c["eps"]).rsqrt()]).float()
    _add(m, "mr_in", mr, "in")  # the backward's mean_rstd: the float64 statistics rounded to fp32
    _add(m, "y", torch.empty(M, C, dtype=TDT[c["tx"]]), "out", lx)
    _add(m, "mean_rstd", torch.empty(2 * C), "out")
    _add(m, "dx", torch.empty(M, C, dtype=TDT[c["tx"]]), "out", lx)
    _add(m, "dgamma", torch.empty(C), "out")
    _add(m, "dbeta", torch.empty(C), "out")
    m["ws_floats"] = None  # the queried size: set by ``add_workspace``
    return m


def add_workspace(c, m, nbytes):
    """BatchNorm: the workspaces of the queried size (one per call), NaN inside, the guard pattern after.  Their
    start is 64 floats in: 8-byte aligned as the FLAT backward needs."""
    m["ws_floats"] = nbytes // 4
    _add(m, "ws_fwd", torch.empty(nbytes // 4), "ws")
    _add(m, "ws_bwd", torch.empty(nbytes // 4), "ws")


def drop_scale(p):
    """1 / (1 - p) as the kernels form it, in fp32."""
    return float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))


# ---------------------------------------------------------------------------------------------- reference

def _ln_v32(c, m):
    """v = fl32(fl32(drop(x) scale) + res) on every row (pad rows: 0), and the fp32 scale."""
    x = view(m, "x").float()
    scale = 1.0
    if c["drop"]:
        scale = drop_scale(c["p"])
        x = torch.where(m["mask"], x * torch.tensor(scale, dtype=torch.float32), torch.zeros(()))
    v = x + view(m, "res").float() if c["res"] else x
    return torch.where(m["live"][:, None], v, torch.zeros(())), scale


def _bf16(dt, ref, bar):
    """The bar of an output stored as ``dt``: rounding a value within ``bar`` of ref to bf16 moves it by at most half
    an ulp, 2^-8 of its magnitude."""
    return bar + 2.0 ** -8 * (ref.abs() + bar) if dt == "bf16" else bar


def ln_reference(c, m):
    """{output: (ref, bar)} in float64 (pad rows of the references are 0)."""
    D = c["D"]
    v32, scale = _ln_v32(c, m)
    v = v32.double()
    live = m["live"][:, None]
    gamma = view(m, "gamma").double()
    mean = v.mean(1, keepdim=True)
    dev = v - mean
    var = (dev ** 2).mean(1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xhat = dev * rstd
    A = mean.abs() + dev.abs().amax(1, keepdim=True)
    cond = D * U * A * rstd
    er = (D + 16) * U + cond ** 2
    ex = cond + xhat.abs() * er
    out = {}
    if not c["bwd"]:
        beta = view(m, "beta").double()
        y = torch.where(live, xhat * gamma + beta, 0.0)
        bar = gamma.abs() * ex + 2 * U * ((gamma * xhat).abs() + beta.abs())
        out["y"] = (y, torch.where(live, _bf16(c["t3"], y, bar), 0.0))
        return out
    dy32 = view(m, "gy").float()
    if c["gy2"]:
        dy32 = dy32 + view(m, "gy2").float()
    dy = torch.where(live, dy32.double(), 0.0)
    gd = gamma * dy
    a1 = gd.abs().mean(1, keepdim=True)
    a2 = (gd * xhat).abs().mean(1, keepdim=True)
    m1 = gd.mean(1, keepdim=True)
    m2 = (gd * xhat).mean(1, keepdim=True)
    gh = torch.where(live, rstd * (gd - m1 - xhat * m2), 0.0)
    em1 = (D + 2) * U * a1
    em2 = (D + 2) * U * a2 + (gd.abs() * ex).mean(1, keepdim=True)
    bar = rstd * ((er + 4 * U) * (gd.abs() + a1 + xhat.abs() * a2) + em1 + ex * a2 + xhat.abs() * em2)
    bar = torch.where(live, bar, 0.0)
    if c["gres"]:
        out["gres"] = (gh, _bf16(c["tr"], gh, bar))
    ghx, barx = gh, bar
    if c["drop"]:
        ghx = torch.where(m["mask"], gh * scale, 0.0)
        barx = torch.where(m["mask"], bar * scale + U * ghx.abs(), 0.0)
    out["gh"] = (ghx, _bf16(c["tx"], ghx, barx))
    R = int(m["live"].sum())
    f = 2 * (R + 8) * U
    t = dy * xhat
    out["dgamma"] = (t.sum(0), f * t.abs().sum(0) + (dy.abs() * torch.where(live, ex, 0.0)).sum(0))
    out["dbeta"] = (dy.sum(0), f * dy.abs().sum(0))
    return out


def bn_depth(r, M):
    rows = M // r["V"] if r["route"] == FLAT else M
    lane = -(-min(r["RB"], rows) // r["RL"])
    if r["route"] == SCALAR:
        return lane + r["RL"] + r["nb"]
    return lane + (r["V"] + 8 if r["route"] == FLAT else r["RL"]) + -(-r["nb"] // 8) + 8


def bn_reference(c, m):
    """{output: (ref, bar)} of the forward (y, mean_rstd, run_mean, run_var) and the backward (dx, dgamma, dbeta)."""
    M, C, eps, mom = c["M"], c["C"], c["eps"], c["momentum"]
    x = view(m, "x").double()
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gamma = view(m, "gamma").double() if c["affine"] else one
    beta = view(m, "beta").double() if c["affine"] else zero
    mean = x.mean(0)
    dev = x - mean
    var = (dev ** 2).mean(0)
    rstd = (var + eps).rsqrt()
    xhat = dev * rstd
    k = 4 * bn_depth(record(c, "fwd"), M)
    md = dev.abs().amax(0)
    bm = k / 2 * U * (mean.abs() + 2 * md)
    ev = k * U * (var + 2 * md ** 2) + 4 * md * bm
    er = ev / (var + eps) / 2 + 4 * U
    out = {}
    y = xhat * gamma + beta
    out["y"] = (y, _bf16(c["tx"], y, gamma.abs() * (bm * rstd + xhat.abs() * er) +
                         3 * U * ((gamma * xhat).abs() + beta.abs())))
    out["mean_rstd"] = (torch.cat([mean, rstd]), torch.cat([bm, rstd * er]))
    if c["running"]:
        rm, rv = view(m, "run_mean", m["orig"]).double(), view(m, "run_var", m["orig"]).double()
        unb = var * M / (M - 1) if M > 1 else var
        out["run_mean"] = ((1 - mom) * rm + mom * mean, mom * bm + 3 * U * (rm.abs() + mean.abs()))
        out["run_var"] = ((1 - mom) * rv + mom * unb,
                          mom * ev * (M / (M - 1) if M > 1 else 1.0) + 3 * U * (rv.abs() + unb.abs()))
    # backward: mean_rstd as given
    mr = view(m, "mr_in").double()
    mu, rs = mr[:C], mr[C:]
    dy = view(m, "dy").double()
    xh = (x - mu) * rs
    t = dy * xh
    dbeta, dgamma = dy.sum(0), t.sum(0)
    gr = gamma * rs
    dx = gr * (dy - dbeta / M - xh * dgamma / M)
    mag = gr.abs() * (dy.abs() + dbeta.abs() / M + (xh * dgamma).abs() / M)
    if record(c, "bwd")["route"] == FLAT:
        h = 2.0 ** -8 if c["tx"] == "bf16" else U
        out["dx"] = (dx, h * dx.abs() + 2.0 ** -48 * mag)
        out["dgamma"] = (dgamma, U * dgamma.abs() + 2.0 ** -48 * t.abs().sum(0))
        out["dbeta"] = (dbeta, U * dbeta.abs() + 2.0 ** -48 * dy.abs().sum(0))
        return out
    f = 2 * (M + 8) * U
    bb = f * dy.abs().sum(0)
    bg = (f + 3 * U) * t.abs().sum(0)
    out["dgamma"], out["dbeta"] = (dgamma, bg), (dbeta, bb)
    out["dx"] = (dx, _bf16(c["tx"], dx, 6 * U * mag + gr.abs() * (bb / M + xh.abs() * bg / M)))
    return out


def reference(c, m):
    return ln_reference(c, m) if c["kind"] == "ln" else bn_reference(c, m)


# ---------------------------------------------------------------------------------------------- verify

def well_conditioned(c):
    return c["profile"] not in ILL


def rel_l2(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


WHOLE = ("y", "gh", "gres", "dx", "dgamma", "dbeta")


def verify(c, m, ref, report=None):
    """Checks in the order of FAILURES, naming the first that fails.  Returns (worst error / bar, {output: rel-L2});
    report (a dict): filled with the per-output error / bar ratios."""
    nm = c["name"]
    for name, (lo, shape, kind) in m["spec"].items():
        buf = m["bufs"][name]
        n = math.prod(shape)
        if kind == "in":
            assert torch.equal(_bits(buf), _bits(m["orig"][name])), f"{nm}: operand: {name} changed"
            continue
        pat = Y_GUARD.get(buf.dtype, 0x5A5AA5A5)
        bad = _bits(buf) != pat
        bad[lo:lo + n] = False
        assert not bool(bad.any()), f"{nm}: guard: {name}[{int(bad.nonzero()[0]) - lo}] written (tensor of {n})"
    outs = {k: view(m, k) for k in ref}
    if c["kind"] == "ln":
        dead = ~m["live"]
        for k in ("y", "y16", "gh", "gres"):
            if k in m["spec"] and bool(dead.any()):
                rows = _bits(view(m, k))[dead]
                first = rows.any(1).nonzero()
                assert not bool(rows.any()), f"{nm}: pad row: {k} row {int(dead.nonzero()[int(first[0])])} is not zero"
    for k, v in outs.items():
        fin = torch.isfinite(v.float())
        assert bool(fin.all()), f"{nm}: non-finite: {int((~fin).sum())} elements of {k}"
    if "y16" in m["spec"]:
        assert torch.equal(_bits(view(m, "y16")), _bits(view(m, "y").bfloat16())), f"{nm}: copy: y16 is not bf16(y)"
    if "nbt" in m["spec"]:
        assert int(view(m, "nbt")[0]) == int(view(m, "nbt", m["orig"])[0]) + 1, f"{nm}: num_batches: not old + 1"
    worst, rels, ratios = 0.0, {}, {}
    for k, v in outs.items():
        r, bar = ref[k]
        err = (v.double() - r).abs()
        ratio = float((err / bar.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
        worst = max(worst, ratio)
        ratios[k] = ratio
        if report is not None:
            report[k] = ratio
        over = err > bar
        assert not bool(over.any()), f"{nm}: element bar: {int(over.sum())} of {over.numel()} elements of {k} over " \
                                     f"(worst ratio {ratio:.3g}), first at {tuple(int(i) for i in over.nonzero()[0])}"
    for k, v in outs.items():
        if k not in WHOLE:
            continue
        rels[k] = rel_l2(v.double(), ref[k][0])
        if well_conditioned(c):
            tol = REL_L2_F32 if v.dtype == torch.float32 else REL_L2_BF16
        else:
            assert c["ill"] and k in c["ill"], f"{nm}: rel-L2: no stand-in value recorded for {k}"
            tol = 4 * c["ill"][k] + (REL_L2_BF16 if v.dtype == torch.bfloat16 else 0.0)
        assert rels[k] <= tol, f"{nm}: rel-L2: {k} {rels[k]:.3e} > {tol:.3e}"
    print(f"{nm}: worst error/bar {worst:.3e} (" + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()) +
          "), rel-L2 " + " ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    return worst, rels


# ---------------------------------------------------------------------------------------------- stand-in

def applies(c, mutate):
    """Whether the fault changes anything the checker can see on this case."""
    if c["kind"] == "ln":
        lens = lens_of(c)
        pad = lens is not None and any(n < c["T"] for n in lens)
        live = c["B"] * c["T"] if lens is None else sum(lens)
        rows = c["B"] * c["T"]
        last_live = lens is None or lens[-1] == c["T"]
        return {"one_pass_var": c["profile"] == "offset" and c["tx"] == "f32" or
                (c["profile"] == "offset" and c["res"] and c["tr"] == "f32"),
                "pad_row_live": pad, "mask_off_by_one": pad,
                "drop_partial": c["bwd"] and ln_nblk(c) > 1 and last_live and live <= R_MAX and
                c["profile"] in ("plain", "tiny"),
                "row_shift": (lens is None or lens[0] >= 2) and c["T"] >= 2 and c["profile"] == "plain",
                "no_gy2": c["gy2"], "drop_unscaled": c["drop"] and c["p"] > 0,
                "write_past": True}.get(mutate, False)
    return {"one_pass_var": c["profile"] == "offset" and c["tx"] == "f32" and c["M"] > 1,
            "shift_first_outlier": c["profile"] == "offset" and c["tx"] == "f32" and c["M"] > 1 and
            record(c, "fwd")["route"] == VEC,
            "biased_running_var": c["running"] and 1 < c["M"] <= 200 and c["profile"] == "plain",  # 1 / M over the bar
            "write_past": True}.get(mutate, False)


def _ln_standin(c, m, mutate):
    D = c["D"]
    x = view(m, "x").float()
    live = m["live"].clone()
    rows = live.numel()
    if mutate == "mask_off_by_one":  # t > lens: row t == lens[b] counts as live
        lens = torch.tensor(lens_of(c))
        live = (torch.arange(c["T"])[None, :] <= lens[:, None]).reshape(rows)
    if mutate == "pad_row_live":
        live[int((~live).nonzero()[0])] = True
    scale = torch.tensor(1.0)
    if c["drop"]:
        scale = torch.tensor(drop_scale(c["p"]), dtype=torch.float32)
        x = torch.where(m["mask"], x if mutate == "drop_unscaled" else x * scale, torch.zeros(()))
    v = x + view(m, "res").float() if c["res"] else x
    mean = v.mean(1, keepdim=True)
    if mutate == "one_pass_var":
        var = ((v * v).mean(1, keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    if mutate == "row_shift":  # row 1 normalised with row 0's statistics
        mean, rstd = mean.clone(), rstd.clone()
        mean[1], rstd[1] = mean[0], rstd[0]
    xhat = (v - mean) * rstd
    gamma = view(m, "gamma")
    lv = live[:, None]
    if not c["bwd"]:
        y = torch.where(lv, xhat * gamma + view(m, "beta"), torch.zeros(()))
        view(m, "y").copy_(y.to(view(m, "y").dtype))
        if c["dual"]:
            view(m, "y16").copy_(view(m, "y").bfloat16())
        last = "y"
    else:
        dy = view(m, "gy").float()
        if c["gy2"] and mutate != "no_gy2":
            dy = dy + view(m, "gy2").float()
        dy = torch.where(lv, dy, torch.zeros(()))
        xhat = torch.where(lv, xhat, torch.zeros(()))
        gd = gamma * dy
        m1, m2 = gd.mean(1, keepdim=True), (gd * xhat).mean(1, keepdim=True)
        gh = torch.where(lv, rstd * (gd - m1 - xhat * m2), torch.zeros(()))
        if c["gres"]:
            view(m, "gres").copy_(gh.to(view(m, "gres").dtype))
        if c["drop"]:
            gh = torch.where(m["mask"], gh if mutate == "drop_unscaled" else gh * scale, torch.zeros(()))
        view(m, "gh").copy_(gh.to(view(m, "gh").dtype))
        # per-workgroup partials of 64 rows in the kernels' workspace layout [nblk][2][D], added in order
        nblk = ln_nblk(c)
        ws = view(m, "ws").view(nblk, 2, D)
        padded = torch.zeros(nblk * 64, 2, D)
        padded[:rows, 0], padded[:rows, 1] = dy * xhat, dy
        ws.copy_(padded.view(nblk, 64, 2, D).sum(1))
        tot = ws[:nblk - (mutate == "drop_partial")].sum(0)
        view(m, "dgamma").copy_(tot[0])
        view(m, "dbeta").copy_(tot[1])
        last = "gh"
    if mutate == "write_past":
        lo, shape, _ = m["spec"][last]
        b = _bits(m["bufs"][last])
        b[lo + math.prod(shape)] += 1


def _bn_standin(c, m, mutate):
    M, C, eps, mom = c["M"], c["C"], c["eps"], c["momentum"]
    x = view(m, "x").float()
    gamma = view(m, "gamma") if c["affine"] else torch.ones(C)
    beta = view(m, "beta") if c["affine"] else torch.zeros(C)
    mean = x.mean(0)
    if mutate == "one_pass_var":
        var = ((x * x).mean(0) - mean * mean).clamp_min(0)
    elif mutate == "shift_first_outlier":  # each row lane sums v and v^2 as they are; the lanes merged exactly
        RL = min(record(c, "fwd")["RL"], M)
        n = torch.tensor([len(range(l, M, RL)) for l in range(RL)], dtype=torch.float32)[:, None]
        a1 = torch.stack([x[l::RL].sum(0) for l in range(RL)])
        a2 = torch.stack([(x[l::RL] * x[l::RL]).sum(0) for l in range(RL)])
        m2 = (a2 - a1 * a1 / n).double()
        lm = (a1 / n).double()
        mean64 = (lm * n.double()).sum(0) / M
        var = ((m2.sum(0) + (n.double() * (lm - mean64) ** 2).sum(0)) / M).clamp_min(0).float()
        mean = mean64.float()
    else:
        var = ((x - mean) ** 2).mean(0)
    rstd = (var + eps).rsqrt()
    y = (x - mean) * rstd * gamma + beta
    view(m, "y").copy_(y.to(view(m, "y").dtype))
    view(m, "mean_rstd").copy_(torch.cat([mean, rstd]))
    if c["running"]:
        unb = var * (M / (M - 1)) if M > 1 and mutate != "biased_running_var" else var
        view(m, "run_mean").mul_(1 - mom).add_(mom * mean)
        view(m, "run_var").mul_(1 - mom).add_(mom * unb)
        view(m, "nbt").add_(1)
    mr = view(m, "mr_in")
    flat = record(c, "bwd")["route"] == FLAT
    wd = torch.float64 if flat else torch.float32  # the FLAT backward works in double and rounds once
    mu, rs, dy, xw, gw = mr[:C].to(wd), mr[C:].to(wd), view(m, "dy").to(wd), view(m, "x").to(wd), gamma.to(wd)
    xh = (xw - mu) * rs
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    dx = gw * rs * (dy - dbeta / M - xh * dgamma / M)
    view(m, "dx").copy_(dx.to(view(m, "dx").dtype))
    view(m, "dgamma").copy_(dgamma.float())
    view(m, "dbeta").copy_(dbeta.float())
    if mutate == "write_past":
        lo, shape, _ = m["spec"]["dx"]
        b = _bits(m["bufs"]["dx"])
        b[lo + math.prod(shape)] += 1


def standin(c, m, mutate=None):
    """The CPU stand-in for the kernels in the self-test: plain fp32 torch in the kernels' formulation (two-pass
    LayerNorm, per-workgroup dgamma partials; BatchNorm statistics about the mean), written into the guarded
    views.  ``mutate`` names a deliberate fault (MUTATIONS)."""
    (_ln_standin if c["kind"] == "ln" else _bn_standin)(c, m, mutate)


def old_rel_l2(c, m, ref):
    """The largest whole-tensor rel-L2 over the outputs: what the superseded tests compared with 1e-2 / 1e-5."""
    return max(rel_l2(view(m, k).double(), ref[k][0]) for k in ref if k in WHOLE)
