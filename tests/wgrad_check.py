"""Checker of one vo_conv1d_wgrad_bias call (and of vo_colsum) against float64, with a derived element-wise
bar, guard bands around every buffer and the launch record the call must leave.

A case is a dict (see ``case``).  ``make`` draws its operands on the CPU and lays every buffer out with guards,
``reference`` computes the float64 result and the bars, a runner (the GPU test, or in the CPU self-test
``standin``) fills both output sets of the case, and ``verify`` checks guards, operands, values and that the
second run is bit-identical to the first.

    dW[g M + m, n, k] = sum_{b, t < T_A} A[b, t, g M + m] * B[b, t S + k dil - pad, g N + n]

(rows of B outside [0, T_B) are zero; Conv1d: A = dY, B = pre(x); ConvTranspose1d: A = pre(x), B = dY -- the
same sum, which is why one kernel family serves both).

Operands: bf16-exact for bf16 compute; a prologue leaky-ReLU is applied in fp32 and, for bf16, rounded to bf16
as the kernels stage it (lrelu_pack).  Both operands are views into larger buffers: NaN sentinel rows before
the first and after the last utterance, NaN sentinel channels in [groups M, lda) and [groups N, ldb).  dW and
db sit inside buffers pre-filled with a fixed bit pattern; the workspace has the queried size, pre-filled with
NaN (a partial that the reduce reads but no workgroup wrote shows up in dW), plus a guard tail of that pattern.

Element bar: |got - ref| <= 2 (R + 8) 2^-24 A, R = B T_A the reduction length, A the same sum on absolute
values -- the any-order fp32 summation bound of conv_check.py (bf16 products are exact in fp32; the factor 2
covers the fp32 MFMA's product roundings).  Split-bf16 (x3) adds 3 * 2^-18 A, the per-product bound that
tests/test_gpu_f32x3.py documents.  Whole tensor: rel-L2 < 1e-5 (conv_check.REL_L2_F32), x3 < 2e-5 (TOL of
test_gpu_f32x3.py).
Sensitivity: one dropped row moves an element by about A / R, that is 2^23 / R^2 times the element bar; every
case keeps R <= 1200 (``case`` asserts it), so that ratio is at least 5.8.
"""

import contextlib

import torch

FIELDS = ("ROUTE", "TM", "KG", "SW", "ntg", "gpt", "splits", "rows_per_split", "direct", "reduce_W",
          "compute_dtype", "bias")
PER_TAP, MULTI_TAP, K1 = 1, 2, 3
VO_DT = {"f32": 0, "bf16": 1, "x3": 2}
TDT = {"bf16": torch.bfloat16, "f32": torch.float32, "x3": torch.float32}
EV = {"bf16": 8, "f32": 4, "x3": 4}       # elements per 16-byte vector: M, N and the leading dims are multiples
REL_L2 = {"bf16": 1e-5, "f32": 1e-5, "x3": 2e-5}
OLD_BF16_REL_L2 = 1e-2                     # the whole-tensor bar of the bf16 tests this checker supersedes
SLOPE = 0.1
GUARD = 0x5A5AA5A5                         # a fixed bit pattern (a finite fp32, about 1.5e16)
GUARD_N = 64                               # guard floats on each side of dW / db
WS_GUARD_N = 256                           # guard floats after the queried workspace
ROW_GUARD = 8                              # sentinel rows before the first and after the last utterance
R_MAX = 1200
FAILURES = ("guard", "operand", "non-finite", "element bar", "rel-L2", "determinism")


def case(B, T_A, M, N, K, *, S=1, dil=1, pad=0, groups=1, dt="bf16", pre_a=False, pre_b=False, bias=False,
         transposed=False, T_B=None, lda_extra=None, ldb_extra=None, knobs=None, rec=None, name=None, seed=None):
    """One call.  M, N: channels per group of A and B; T_A: rows of A per utterance (T_out of a conv, T_in of a
    transposed conv); T_B None = (T_A - 1) S + dil (K - 1) + 1 - 2 pad, the rows the sum reaches.  transposed:
    the reference goes through conv_transpose1d (A = pre(x), B = dY; dil 1, ungrouped).  lda_extra / ldb_extra:
    sentinel channels past groups M / groups N (None = one 16-byte vector).  knobs: vo_tune values of the call
    (and of its workspace query).  rec: the first ten fields of the launch record the call must leave."""
    ev = EV[dt]
    T_B = (T_A - 1) * S + dil * (K - 1) + 1 - 2 * pad if T_B is None else T_B
    c = dict(B=B, T_A=T_A, T_B=T_B, M=M, N=N, K=K, S=S, dil=dil, pad=pad, groups=groups, dt=dt, pre_a=bool(pre_a),
             pre_b=bool(pre_b), bias=bool(bias), transposed=bool(transposed),
             lda=groups * M + (ev if lda_extra is None else lda_extra),
             ldb=groups * N + (ev if ldb_extra is None else ldb_extra), knobs=dict(knobs or {}), rec=rec)
    R = B * T_A
    assert R <= R_MAX and 2.0 ** 23 / R ** 2 >= 5.8, f"R = {R}: a dropped row would sit too close to the bar"
    assert T_B >= 1 and M % ev == 0 and N % ev == 0 and c["lda"] % ev == 0 and c["ldb"] % ev == 0
    assert not (bias and pre_a), "the fused bias sums A as stored"
    assert not transposed or (dil == 1 and groups == 1 and T_B == (T_A - 1) * S + K - 2 * pad)
    c["seed"] = seed if seed is not None else (B * 1000003 + T_A * 1009 + M * 31 + N * 7 + K * 3 + S) % (2 ** 31)
    kn = "".join(f"_{k}{v}" for k, v in sorted(c["knobs"].items()))
    c["name"] = name or (f"{dt}_B{B}_T{T_A}_M{M}_N{N}_K{K}" + (f"_s{S}" if S > 1 else "") +
                         (f"_d{dil}" if dil > 1 else "") + (f"_p{pad}" if pad else "") +
                         (f"_g{groups}" if groups > 1 else "") + ("_prea" if pre_a else "") +
                         ("_preb" if pre_b else "") + ("_bias" if bias else "") + ("_tr" if transposed else "") + kn)
    return c


def record(c):
    """The launch record the case declares (FIELDS order)."""
    r = dict(zip(FIELDS, c["rec"]))
    r["compute_dtype"] = VO_DT[c["dt"]]
    r["bias"] = int(c["bias"])
    return r


def plan_args(c):
    """Arguments of ops.conv1d_wgrad_plan."""
    return (c["B"], c["T_A"], c["T_B"], c["M"], c["N"], c["K"]), dict(
        S=c["S"], dil=c["dil"], pad=c["pad"], groups=c["groups"], pre_a=c["pre_a"], pre_b=c["pre_b"],
        dtype=VO_DT[c["dt"]], with_bias=c["bias"])


def reached(c):
    """The kernel instantiations and code paths the case exercises, derived from its sizes and its declared
    record (which the CPU suite checks against vo_conv1d_wgrad_plan and the GPU test against the launch)."""
    r = record(c)
    B, T_A, T_B, M, N, K, S, G, dt = (c[k] for k in ("B", "T_A", "T_B", "M", "N", "K", "S", "groups", "dt"))
    R, splits, rps = B * T_A, r["splits"], r["rows_per_split"]
    out = set()
    n_tot = sum(sizes(c)) if c["bias"] else sizes(c)[0]
    if not r["direct"]:
        out.add(f"reduce/W{r['reduce_W']}")
        if n_tot % 64 and n_tot % 256:
            out.add(f"reduce/W{r['reduce_W']}/ragged")
        if c["bias"]:
            out.add(f"reduce/W{r['reduce_W']}/bias")
    if r["ROUTE"] == MULTI_TAP:
        tm, kg, sw = r["TM"], r["KG"], r["SW"]
        out.add(("mt", tm, kg, sw))
        cpb = (T_A + 63) // 64
        out.add(f"mt/chunks_per_split/{min(rps // 64, B * cpb)}")
        last = (T_A - 1) % 64 + 1
        if last in (1, 57):
            out.add(f"mt/last_chunk/{last}")
        if K % kg:
            out.add("mt/short_last_run")
        if (min(kg, K) - 1) * c["dil"] == 64:
            out.add(f"mt/window_limit/SW{sw}")
        if c["dil"] > 64:
            out.add("mt/dil>64")
        if S == 3:
            out.add("mt/S3")
        for flag in ("pre_a", "pre_b"):
            if c[flag]:
                out.add(f"mt/{flag}")
        if G > 1:
            out.add("mt/groups")
        if c["bias"]:
            out.add(f"mt/bias/TM{tm}")
        if M % tm and N % tm:
            out.add(f"mt/partial_tile/TM{tm}")
        return out
    if r["ROUTE"] == K1:
        nch = [(min(R, (s + 1) * rps) - s * rps + 63) // 64 for s in range(splits)]
        out.add("k1/direct" if r["direct"] else "k1/split")
        out.update(f"k1/chunks/{min(n, 3)}" for n in nch)
        if (R - (splits - 1) * rps) % 64 == 1:
            out.add("k1/one_row_tail")
        if M % 128 and N % 128:
            out.add("k1/partial_tile")
        out.add("k1/bias" if c["bias"] else "k1/no_bias")
        return out
    p = f"per_tap/{dt}/"
    out.add(p + ("direct" if r["direct"] else "partials_one_split" if splits == 1 else "splits"))
    if splits > 1 and rps % T_A and (R - (splits - 1) * rps) % 64 == 1:
        out.add(p + "split_inside_utterance_one_row_tail")
    if (M * r["gpt"]) % 64 and (N * r["gpt"]) % 64:
        out.add(p + "partial_tile")
    out.add(p + ("bias" if c["bias"] else "no_bias"))
    if c["pre_b"]:
        out.add(p + "pre_b")
    if c["pad"] > T_B:
        out.add(p + "pad>T")
    if S > 1:
        out.add(p + f"S{S}")
    if G > 1:
        out.add(p + ("gpt>1" if r["gpt"] > 1 else "grouped_gpt1") + ("/bias" if c["bias"] else ""))
    if c["transposed"] and c["pre_a"]:
        out.add(p + "transposed")
    return out


@contextlib.contextmanager
def knobs(c):
    """The vo_tune values of the case, put back to 0 afterwards."""
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    try:
        for k, v in c["knobs"].items():
            assert L.vo_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k in c["knobs"]:
            L.vo_tune(k.encode(), 0)


def sizes(c):
    """(n_w, n_b): floats of dW (groups M, N, K) and of db."""
    return c["groups"] * c["M"] * c["N"] * c["K"], c["groups"] * c["M"]


# ---- views into the guarded buffers (any device)

def a_view(c, buf):
    return buf[ROW_GUARD:ROW_GUARD + c["B"] * c["T_A"], :c["groups"] * c["M"]].unflatten(0, (c["B"], c["T_A"]))


def b_view(c, buf):
    return buf[ROW_GUARD:ROW_GUARD + c["B"] * c["T_B"], :c["groups"] * c["N"]].unflatten(0, (c["B"], c["T_B"]))


def dw_view(c, buf):
    return buf[GUARD_N:GUARD_N + sizes(c)[0]].view(c["groups"] * c["M"], c["N"], c["K"])


def db_view(c, buf):
    return buf[GUARD_N:GUARD_N + sizes(c)[1]]


def _pattern(n):
    return torch.full((n,), GUARD, dtype=torch.int32).view(torch.float32)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _exact(t, c):
    return t.bfloat16().float() if c["dt"] == "bf16" else t


def fresh_out(c, ws_floats):
    n_w, n_b = sizes(c)
    return dict(dw_buf=_pattern(n_w + 2 * GUARD_N), db_buf=_pattern(n_b + 2 * GUARD_N) if c["bias"] else None,
                ws_buf=torch.cat([torch.full((ws_floats,), float("nan")), _pattern(WS_GUARD_N)]))


def make(c):
    """CPU buffers of the case: a_buf / b_buf (rows x ld, the operand views in the middle), their values a_val /
    b_val in fp32, and two output sets (one per run) of dw_buf, db_buf, ws_buf."""
    from visual_onoma_to_wave_amd import _lib
    g = torch.Generator().manual_seed(c["seed"])
    B, T_A, T_B, GM, GN = c["B"], c["T_A"], c["T_B"], c["groups"] * c["M"], c["groups"] * c["N"]
    a = _exact(torch.randn(B, T_A, GM, generator=g), c)
    b = _exact(torch.randn(B, T_B, GN, generator=g), c)
    m = dict(a_val=a, b_val=b)
    for key, v, T, ld in (("a", a, T_A, c["lda"]), ("b", b, T_B, c["ldb"])):
        buf = torch.full((B * T + 2 * ROW_GUARD, ld), float("nan"), dtype=TDT[c["dt"]])
        buf[ROW_GUARD:ROW_GUARD + B * T, :v.shape[2]] = v.reshape(B * T, -1).to(buf.dtype)
        m[key + "_buf"], m[key + "_orig"] = buf, buf.clone()
    with knobs(c):
        ws = int(_lib.lib().vo_conv1d_wgrad_workspace_size(B, T_A, c["M"], c["N"], c["K"], c["groups"])) // 4
    m["ws_floats"] = ws
    m["outs"] = [fresh_out(c, ws), fresh_out(c, ws)]
    return m


def staged(c, x, on):
    """An operand as the kernels stage it: the leaky-ReLU in fp32, rounded to bf16 for bf16 compute."""
    if not on:
        return x.float()
    x = x.float()
    return _exact(torch.maximum(x, x * torch.tensor(SLOPE, dtype=torch.float32)), c)


def _dw64(c, a, b):
    """float64 dW (groups M, N, K) of staged operands a (B, T_A, groups M), b (B, T_B, groups N)."""
    M, N, K, G = c["M"], c["N"], c["K"], c["groups"]
    at, bt = a.double().transpose(1, 2), b.double().transpose(1, 2)
    if c["transposed"]:  # A = x (Ci = M), B = dY (Co = N): the gradient of conv_transpose1d's (Ci, Co, K) weight
        w = torch.zeros(M, N, K, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv_transpose1d(at, w, stride=c["S"], padding=c["pad"])
        return torch.autograd.grad(y, w, bt)[0]
    return torch.nn.grad.conv1d_weight(bt, (G * M, N, K), at, stride=c["S"], padding=c["pad"], dilation=c["dil"],
                                       groups=G)


def reference(c, m):
    """dict(dw, dw_bar, db, db_bar) in float64 (db None without bias)."""
    a, b = staged(c, m["a_val"], c["pre_a"]), staged(c, m["b_val"], c["pre_b"])
    R = c["B"] * c["T_A"]
    f = 2 * (R + 8) * 2.0 ** -24 + (3 * 2.0 ** -18 if c["dt"] == "x3" else 0.0)
    ref = dict(dw=_dw64(c, a, b), dw_bar=f * _dw64(c, a.abs(), b.abs()), db=None, db_bar=None)
    if c["bias"]:
        ref["db"] = m["a_val"].double().sum((0, 1))
        ref["db_bar"] = f * m["a_val"].double().abs().sum((0, 1))
    return ref


def _guards(c, o, ws_floats):
    """(buffer name, index) of the first guard element of an output set that is not the pattern, or None."""
    n_w, n_b = sizes(c)
    for key, n, lo in (("dw_buf", n_w, GUARD_N), ("db_buf", n_b, GUARD_N), ("ws_buf", ws_floats, 0)):
        if o[key] is None:
            continue
        raw = o[key].view(torch.int32)
        bad = raw != GUARD
        bad[lo:lo + n] = False
        if bool(bad.any()):
            return key, int(bad.nonzero()[0])
    return None


def verify(c, m, ref):
    """Checks, in this order and naming the first that fails: guards of both runs bit-identical, operands
    unchanged, everything finite, the element bar, the whole-tensor bar, the second run bit-identical to the
    first.  Returns (worst error / bar, worst rel-L2) over dW and db; raises AssertionError."""
    nm = c["name"]
    for i, o in enumerate(m["outs"]):
        hit = _guards(c, o, m["ws_floats"])
        assert hit is None, f"{nm}: guard: run {i} wrote {hit[0]}[{hit[1]}]" if hit else ""
    for key in ("a", "b"):
        same = torch.equal(_bits(m[key + "_buf"]), _bits(m[key + "_orig"]))
        assert same, f"{nm}: operand: {key}_buf changed"
    o = m["outs"][0]
    got = [("dW", dw_view(c, o["dw_buf"]).double(), ref["dw"], ref["dw_bar"])]
    if c["bias"]:
        got.append(("db", db_view(c, o["db_buf"]).double(), ref["db"], ref["db_bar"]))
    for what, v, _, _ in got:
        assert bool(torch.isfinite(v).all()), f"{nm}: non-finite: {int((~torch.isfinite(v)).sum())} elements of {what}"
    worst, worst_rel = 0.0, 0.0
    for what, v, r, bar in got:
        err = (v - r).abs()
        ratio = float((err / bar.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        over = err > bar
        assert not bool(over.any()), f"{nm}: element bar: {int(over.sum())} of {over.numel()} elements of {what} " \
                                     f"over (worst ratio {ratio:.3g}), first at " \
                                     f"{tuple(int(i) for i in over.nonzero()[0])}"
    for what, v, r, _ in got:
        rel = float((v - r).norm() / r.norm().clamp_min(1e-30))
        worst_rel = max(worst_rel, rel)
        assert rel < REL_L2[c["dt"]], f"{nm}: rel-L2: {what} {rel:.3e} >= {REL_L2[c['dt']]}"
    print(f"{nm}: worst error/bar {worst:.3e}, rel-L2 {worst_rel:.3e}")
    o2 = m["outs"][1]
    same = torch.equal(_bits(dw_view(c, o["dw_buf"])), _bits(dw_view(c, o2["dw_buf"])))
    if c["bias"]:
        same = same and torch.equal(_bits(db_view(c, o["db_buf"])), _bits(db_view(c, o2["db_buf"])))
    assert same, f"{nm}: determinism: the second run differs from the first"
    return worst, worst_rel


def old_bf16_rel_l2(c, m, ref):
    """rel-L2 of the first run's dW: what the superseded bf16 tests compared with OLD_BF16_REL_L2."""
    v = dw_view(c, m["outs"][0]["dw_buf"]).double()
    return float((v - ref["dw"]).norm() / ref["dw"].norm().clamp_min(1e-30))


# ---- the CPU stand-in for the kernels, and its deliberate faults

# The row faults act on the last tap.  drop_row: the first in-range row of the last utterance is dropped.
# leak_row: rows outside [0, T_B) read the neighbouring utterance (where there is one) instead of zero.  shift_tap:
# the tap's bound test is one row late while its load is clamped -- the row one past the end reads row T_B - 1,
# row 0 reads zero.  stride_as_one: the tap walks B with stride 1.  leak_channel: the last channel of A is read
# one vector too far (channel groups M of lda, a sentinel).  off_diagonal: group 1's block is computed from group
# 0's B columns (what a packed tile keeps if it keeps the wrong block).  drop_split: the reduce leaves out the last
# split.  unwritten_partial: 16 floats of the last split's partial are never written.  bias_misses_tail: db misses
# the last row.  guard_*: one element past dW, before db, past the queried workspace.  touch_operand: B is written.
# scale: everything off by 3e-5 relative (under the element bar at R >= 286, over the whole-tensor bar).
# second_run_differs: one ulp on one element of the second run.
MUTATIONS = {  # name -> the failure verify must name
    "drop_row": "element bar", "leak_row": "element bar", "shift_tap": "element bar",
    "stride_as_one": "element bar", "leak_channel": "non-finite", "off_diagonal": "element bar",
    "drop_split": "element bar", "unwritten_partial": "non-finite", "bias_misses_tail": "element bar",
    "guard_dw": "guard", "guard_db": "guard", "guard_ws": "guard", "touch_operand": "operand",
    "scale": "rel-L2", "second_run_differs": "determinism"}


def applies(c, mutate):
    """Whether the fault changes anything on this case."""
    split = not record(c)["direct"] and min(c["B"], record(c)["splits"]) > 1
    k = c["K"] - 1
    tb = [t * c["S"] + k * c["dil"] - c["pad"] for t in range(c["T_A"])]
    inside = any(0 <= v < c["T_B"] for v in tb)
    edge = any(v in (0, c["T_B"]) for v in tb)
    outside = any(-c["T_B"] <= v < 0 or c["T_B"] <= v < 2 * c["T_B"] for v in tb)
    return {"stride_as_one": c["S"] > 1 and c["T_A"] > 1, "off_diagonal": record(c)["gpt"] > 1,
            "drop_split": split, "unwritten_partial": split, "bias_misses_tail": c["bias"], "guard_db": c["bias"],
            "drop_row": inside, "shift_tap": edge, "leak_row": outside and c["B"] > 1,
            "scale": 2 * (c["B"] * c["T_A"] + 8) * 2.0 ** -24 > 3.5e-5}.get(mutate, True)


def _tap(c, a_u, b_all, u, k, mutate):
    """(groups M, N) of tap k and utterance u from the staged fp32 operands (b_all: every utterance), with the
    row faults: the gather form of the sum in the module docstring."""
    T_A, T_B, M, N, G = c["T_A"], c["T_B"], c["M"], c["N"], c["groups"]
    t = torch.arange(T_A)
    S = 1 if mutate == "stride_as_one" else c["S"]
    tb = t * S + k * c["dil"] - c["pad"]
    ok = (tb >= 0) & (tb < T_B)
    if mutate == "shift_tap":  # the bound test one row late, the load clamped: row T_B reads row T_B - 1, row 0 zero
        ok = (tb >= 1) & (tb <= T_B)
    flat = b_all.reshape(-1, b_all.shape[2])
    if mutate == "leak_row":  # the neighbouring utterance's rows, where there is one
        q = u * T_B + tb
        ok = (q >= 0) & (q < flat.shape[0]) & (tb > -T_B) & (tb < 2 * T_B)
        rows = flat[q.clamp(0, flat.shape[0] - 1)] * ok[:, None]
    else:
        rows = flat[u * T_B + tb.clamp(0, T_B - 1)] * ok[:, None]
    a_u = a_u.clone()
    if mutate == "drop_row" and u == c["B"] - 1 and bool(ok.any()):
        a_u[int(ok.nonzero()[0])] = 0
    return torch.cat([a_u[:, g * M:(g + 1) * M].T @ rows[:, g * N:(g + 1) * N] for g in range(G)])


def _standin_dw(c, a, b, mutate):
    """Per-utterance fp32 dW (B, groups M, N, K): conv1d_weight, the faulty tap from the gather form."""
    M, N, K, G = c["M"], c["N"], c["K"], c["groups"]
    out = []
    for u in range(c["B"]):
        at, bt = a[u:u + 1].transpose(1, 2), b[u:u + 1].transpose(1, 2)
        dw = torch.nn.grad.conv1d_weight(bt, (G * M, N, K), at, stride=c["S"], padding=c["pad"], dilation=c["dil"],
                                         groups=G)
        if mutate in ("drop_row", "leak_row", "shift_tap", "stride_as_one"):
            dw[:, :, K - 1] = _tap(c, a[u], b, u, K - 1, mutate)
        if mutate == "off_diagonal":  # group 1's block from group 0's B columns
            dw[M:2 * M] = torch.nn.grad.conv1d_weight(bt[:, :N], (M, N, K), at[:, M:2 * M], stride=c["S"],
                                                      padding=c["pad"], dilation=c["dil"])
        out.append(dw)
    return torch.stack(out)


def _standin_once(c, m, o, mutate, second):
    B, T_A, M, N, K, G = c["B"], c["T_A"], c["M"], c["N"], c["K"], c["groups"]
    n_w, n_b = sizes(c)
    av, bv = a_view(c, m["a_buf"]), b_view(c, m["b_buf"])
    if mutate == "leak_channel":  # the last channel of A read one vector too far: channel groups M of lda
        av = m["a_buf"][ROW_GUARD:ROW_GUARD + B * T_A].unflatten(0, (B, T_A))[
            :, :, list(range(G * M - 1)) + [G * M]]
    a, b = staged(c, av, c["pre_a"]), staged(c, bv, c["pre_b"])
    dws = _standin_dw(c, a, b, mutate)
    if mutate == "scale":
        dws = dws * (1 + 3e-5)
    dbs = av.float().sum(1)  # (B, groups M)
    if mutate == "bias_misses_tail":
        dbs[-1] -= av[-1, -1].float()
    rec = record(c)
    nsp = 1 if rec["direct"] else min(B, rec["splits"])
    if rec["direct"]:  # summed in utterance order, written in the final layout
        dw, db = dws[0].clone(), dbs[0].clone()
        for u in range(1, B):
            dw, db = dw + dws[u], db + dbs[u]
    else:  # tap-major partials [split][group][K][M][N] + [groups M] in the workspace, then added in split order
        n_tot = n_w + (n_b if c["bias"] else 0)
        ws = o["ws_buf"]
        for s, us in enumerate(torch.arange(B).tensor_split(nsp)):
            pw, pb = dws[int(us[0])].clone(), dbs[int(us[0])].clone()
            for u in us[1:]:
                pw, pb = pw + dws[int(u)], pb + dbs[int(u)]
            ws[s * n_tot:s * n_tot + n_w] = pw.view(G, M, N, K).permute(0, 3, 1, 2).reshape(-1)
            if c["bias"]:
                ws[s * n_tot + n_w:(s + 1) * n_tot] = pb
        if mutate == "unwritten_partial":
            ws[(nsp - 1) * n_tot + n_w - 16:(nsp - 1) * n_tot + n_w] = float("nan")
        tot = ws[:n_tot].clone()
        for s in range(1, nsp - (mutate == "drop_split")):
            tot = tot + ws[s * n_tot:(s + 1) * n_tot]
        dw = tot[:n_w].view(G, K, M, N).permute(0, 2, 3, 1).reshape(G * M, N, K)
        db = tot[n_w:]
    if mutate == "second_run_differs" and second:
        dw = dw.clone()
        dw[0, 0, 0] = torch.nextafter(dw[0, 0, 0], torch.tensor(float("inf")))
    dw_view(c, o["dw_buf"]).copy_(dw)
    if c["bias"]:
        db_view(c, o["db_buf"]).copy_(db)
    if mutate == "guard_dw":
        o["dw_buf"].view(torch.int32)[GUARD_N + n_w] += 1
    if mutate == "guard_db":
        o["db_buf"].view(torch.int32)[GUARD_N - 1] += 1
    if mutate == "guard_ws":
        o["ws_buf"].view(torch.int32)[m["ws_floats"]] += 1
    if mutate == "touch_operand":
        m["b_buf"][ROW_GUARD, 0] += 1


def standin(c, m, mutate=None):
    """The CPU stand-in for the kernels in the self-test: fp32 conv1d_weight per utterance, summed in utterance
    order (through workspace partials in the kernels' layout unless the record says ``direct``), on the
    operands as laid out in memory -- read through the views with their leading dimensions.  Fills both output
    sets.  ``mutate`` names a deliberate fault (MUTATIONS)."""
    for i, o in enumerate(m["outs"]):
        _standin_once(c, m, o, mutate, i == 1)


# ---- vo_colsum: out[c] = sum_r x[r, c]

def colsum_case(rows, C, dt, ld_extra=8):
    return dict(rows=rows, C=C, dt=dt, ld=C + ld_extra, name=f"colsum_{dt}_rows{rows}_C{C}",
                seed=(rows * 1009 + C * 31 + len(dt)) % (2 ** 31))


def colsum_make(c):
    """x_buf (sentinel rows around, sentinel channels in [C, ld)), out_buf and ws_buf with guards."""
    from visual_onoma_to_wave_amd import _lib
    g = torch.Generator().manual_seed(c["seed"])
    x = _exact(torch.randn(c["rows"], c["C"], generator=g), c)
    buf = torch.full((c["rows"] + 2 * ROW_GUARD, c["ld"]), float("nan"), dtype=TDT[c["dt"]])
    buf[ROW_GUARD:ROW_GUARD + c["rows"], :c["C"]] = x.to(buf.dtype)
    ws = int(_lib.lib().vo_colsum_workspace_size(c["rows"], c["C"])) // 4
    return dict(x_val=x, x_buf=buf, x_orig=buf.clone(), ws_floats=ws, outs=[
        dict(out_buf=_pattern(c["C"] + 2 * GUARD_N),
             ws_buf=torch.cat([torch.full((ws,), float("nan")), _pattern(WS_GUARD_N)])) for _ in range(2)])


def colsum_view(c, buf):
    return buf[ROW_GUARD:ROW_GUARD + c["rows"], :c["C"]]


def colsum_verify(c, m):
    """The same checks and bar as ``verify`` (R = rows, A = column sums of |x|)."""
    nm, C = c["name"], c["C"]
    for i, o in enumerate(m["outs"]):
        for key, lo, n in (("out_buf", GUARD_N, C), ("ws_buf", 0, m["ws_floats"])):
            bad = o[key].view(torch.int32) != GUARD
            bad[lo:lo + n] = False
            assert not bool(bad.any()), f"{nm}: guard: run {i} wrote {key}[{int(bad.nonzero()[0])}]"
    assert torch.equal(_bits(m["x_buf"]), _bits(m["x_orig"])), f"{nm}: operand: x_buf changed"
    got = m["outs"][0]["out_buf"][GUARD_N:GUARD_N + C].double()
    assert bool(torch.isfinite(got).all()), f"{nm}: non-finite"
    ref = m["x_val"].double().sum(0)
    bar = 2 * (c["rows"] + 8) * 2.0 ** -24 * m["x_val"].double().abs().sum(0)
    err = (got - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    print(f"{nm}: worst error/bar {ratio:.3e}, rel-L2 {rel:.3e}")
    assert not bool((err > bar).any()), f"{nm}: element bar: worst ratio {ratio:.3g}"
    assert rel < REL_L2[c["dt"]], f"{nm}: rel-L2: {rel:.3e}"
    again = m["outs"][1]["out_buf"][GUARD_N:GUARD_N + C]
    assert torch.equal(_bits(m["outs"][0]["out_buf"][GUARD_N:GUARD_N + C]), _bits(again)), f"{nm}: determinism"
    return ratio, rel
