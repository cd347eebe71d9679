"""Checker of one attention forward or backward call against float64, with derived element-wise bars and
guard bands (the attention twin of tests/conv_check.py).

A case is a dict (see ``case``).  ``make`` draws its operands on the CPU and lays the outputs out inside
guarded buffers, ``reference_fwd`` / ``reference_bwd`` compute the float64 result and the bar, the GPU test
(or, in the CPU self-test, ``emulate_fwd`` / ``emulate_bwd``) fills the output views and ``verify`` checks
values, guards and inputs.

Operands: every operand is exact in the dtype under test (drawn in fp32, rounded to bf16 before the
reference sees it).

lens contract (include/vonoma.h): utterance b has n = clamp(lens[b], 0, L) keys, lens = None means L; an
utterance with no key has zero output rows, lse = +inf and zero gradients.

Forward reference, float64 per (b, h): S = scale Q K^T with keys >= n at -inf, P = softmax(S), O = P V,
lse = logsumexp(S); n = 0 gives O = 0 and lse = +inf.

Backward reference: the float64 backward as a function of (qkv, o_in, dout), o_in the forward output in the
dtype actually handed to the kernel: D = rowsum(dO o o_in), dP = dO V^T, dS = P o (dP - D),
dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.  Defined on o_in, the rounding of O is not part of the
error budget; on the CPU it differs from the autograd of the exact forward by rel-L2 <= 2.7e-3 in bf16 and
<= 4e-8 in fp32 (the rounding of o_in itself).

Bars.  f = 2^-24 (fp32 half ulp), u = 2^-8 for bf16 and 2^-24 for fp32, dk = 128, n_t = ceil(n / 64),
spread_i = max_j S_ij - min_{valid j} S_ij, A = P |V|.
  * Relative error of an unnormalised weight exp(s_ij - m_i), on valid keys:
      Delta_ij = 2 (dk + 8) f scale (|Q| |K|^T)_ij        the any-order fp32 dot product q_i . k_j (as in
                                                          conv_check: + 8 the scale multiply, factor 2
                                                          accumulator adds that truncate); an absolute error
                                                          of the score, so a relative one of its exponential
                 + (2 spread_i + 4 (n_t + 1)) 2 f         the __expf argument: the subtraction s - m and the
                                                          scaling by log2(e) each round a number of magnitude
                                                          <= spread (2 spread f each way of counting the
                                                          constant's own rounding); per key tile one hardware
                                                          exp2 (1 ulp = 2 f), one rescale by alpha (its exp2
                                                          and its product) -- 4 roundings of 2 f per tile, + 1
                                                          tile for the weight's own exponential.
    eps_ij = 1.5 (Delta_ij + sum_k p_ik Delta_ik) is the relative error of p_ij = weight / sum: numerator
    plus denominator, 1.5 the linearisation of exp(x) - 1 <= 1.5 x (x <= 0.5, asserted).
  * Forward: bar = 1.5 ((P o Delta) |V| + (sum p Delta) A)     weights and denominator into O
                 + 4 (n + 64) f A       the two any-order fp32 sums over the n keys padded to whole tiles:
                                        sum p v (2 (n + 64) f) and the running sum l (2 (n + 64) f)
                 + 3 f |ref|            the reciprocal (1 ulp) and the product of the normalisation
                 + u |ref|              the output rounded to the dtype
                 + u A  (bf16)          P rounded to a bf16 MFMA operand (the sum l is taken unrounded).
  * lse: bar = 1.5 sum p Delta + R,  R = 2 (n + 64) f    the sum l
                                       + 3 f log max(n, 2)   hardware log2 (1 ulp) and the product with ln 2
                                                             of l in [1, n]
                                       + f |lse|             the add m + log l.
    The running max cancels between m and log l; its effect on the weights is in Delta.
  * Backward: P is rebuilt as exp(s - lse), so eps gains R (the sum behind lse), f |lse| (lse stored as
    fp32) and f (|s| + |lse|) (the subtraction): eps' = eps + R + 2 f (|S| + |lse|).
      e_dS = P o (eps' |dP - D| + 2 (dk + 8) f (|dO| |V|^T + sum |dO| |o_in|))    the two fp32 dot products
             dP and D (the subtraction's own rounding is under the per-tile roundings of Delta)
             + u (|dS| + e_dS)  (bf16)                     dS rounded to a bf16 operand
      bar_dQ = scale (e_dS |K| + 2 (L + 64) f |dS| |K|) + u |dQ|      any-order sum over the keys; the
                                                                    + 64 holds the scale multiply; output
      bar_dK = scale (e_dS^T |Q| + 2 (L + 64) f |dS|^T |Q|) + u |dK|
      bar_dV = (P o eps' (+ u P))^T |dO| + 2 (L + 64) f P^T |dO| + u |dV|
    A masked key has P = 0, so its dK / dV bars are 0: exact zeros are required there (poison_pad, n = 0).
    L = 1 needs no special case: the reference dQ and dK are exactly 0 and the bar is the absolute e_dS term.

Per-row bar (flat draw only): the worst rel-L2 of one (b, row, h) vector of 128 against the project's
tolerances applied per row: forward 2e-5 fp32 / 1e-2 bf16, backward 1e-4 / 2e-2 for rows whose reference is
non-zero (norm above 2^-40 of the same sum on absolute values: below that the float64 reference is its own
rounding noise, e.g. dQ of a row with a single key).  Peaked and ramp draws are judged by the element bar
alone: dP - D cancels there and no per-row relative number is honest.

``emulate_*`` is the kernels' arithmetic in torch on the CPU: fp32 matmuls, 64-key tiles with a running max
and sum, P (and dS) rounded to bf16 before the second product in bf16 mode, the sum taken from the
unrounded P, the output rounded to the dtype.  It shows that the bars admit a correct implementation
(tests/test_attn_check.py); it is never the expected value of a GPU test.
"""

import math

import torch

DK = 128
KT = 64
F = 2.0 ** -24
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
ROW_TOL = {("fwd", "f32"): 2e-5, ("fwd", "bf16"): 1e-2, ("bwd", "f32"): 1e-4, ("bwd", "bf16"): 2e-2}
GUARD = {torch.float32: 0x5A5AA5A5, torch.bfloat16: 0x5A5B}  # a fixed bit pattern (finite in both formats)
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
G = 256  # guard elements on either side of a view (keeps the views 16-byte aligned)
DRAWS = ("flat", "peaked", "ramp_up", "ramp_down", "poison_pad")
POISON = 8192.0
FWD_MUTATIONS = ("extra_key", "drop_last_key", "zero_pad_keys", "no_rescale", "row_swap", "head_swap", "guard")
BWD_MUTATIONS = ("no_D", "padded_key_grad", "drop_last_query", "unscaled_dq", "guard")


def case(B, L, H, lens, draw="flat", dt="bf16", kind="fwd"):
    """lens: a list of B ints or None.  kind: 'fwd' or 'bwd'."""
    assert draw in DRAWS and dt in DT and kind in ("fwd", "bwd") and (lens is None or len(lens) == B)
    ltxt = "none" if lens is None else "-".join(str(n) for n in lens)
    return dict(B=B, L=L, H=H, lens=None if lens is None else list(lens), draw=draw, dt=dt, kind=kind,
                seed=(B * 1000003 + L * 1009 + H * 31 + DRAWS.index(draw)) % (2 ** 31),
                name=f"{kind}-{dt}-{draw}_B{B}_L{L}_H{H}_lens{ltxt}")


def key_counts(c):
    """n_b = clamp(lens[b], 0, L), or L without lens."""
    return [c["L"]] * c["B"] if c["lens"] is None else [min(max(n, 0), c["L"]) for n in c["lens"]]


def _guarded(n, dtype):
    buf = torch.empty(n + 2 * G, dtype=dtype)
    buf.view(_INT[dtype]).fill_(GUARD[dtype])
    return buf


def make(c):
    """CPU operands of the case: qkv (B, L, 3D), dout (B, L, D), lens (int32 or None) and the guarded output
    buffers out / lse / dqkv / ws with their views."""
    g = torch.Generator().manual_seed(c["seed"])
    B, L, H, dt = c["B"], c["L"], c["H"], DT[c["dt"]]
    D = H * DK
    qkv = torch.randn(B, L, 3 * D, generator=g)
    dout = torch.randn(B, L, D, generator=g)
    dirs = torch.randn(H, DK, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    draw = c["draw"]
    if draw == "peaked":
        qkv[:, :, :2 * D] *= 2
    if draw in ("ramp_up", "ramp_down"):
        n_t = (L + KT - 1) // KT
        step = min(8.0, 60.0 / max(n_t - 1, 1))  # total spread of the tile maxima capped at 60
        a = 16.0
        tile = torch.arange(L) // KT
        tile = tile if draw == "ramp_up" else n_t - 1 - tile
        coef = step * tile.float() / (a / DK ** 0.5)
        for h in range(H):
            qkv[:, :, h * DK:(h + 1) * DK] += a * dirs[h]
            qkv[:, :, D + h * DK:D + (h + 1) * DK] += coef[:, None] * dirs[h]
    if draw == "poison_pad":
        sign = 1.0 - 2.0 * ((torch.arange(L)[:, None] + torch.arange(2 * D)[None, :]) % 2).float()
        for b, n in enumerate(key_counts(c)):
            qkv[b, n:, D:] = POISON * sign[n:]
    m = dict(qkv=qkv.to(dt), dout=dout.to(dt))
    m["lens"] = None if c["lens"] is None else torch.tensor(c["lens"], dtype=torch.int32)
    for name, shape, t in (("out", (B, L, D), dt), ("lse", (B, H, L), torch.float32), ("dqkv", (B, L, 3 * D), dt),
                           ("ws", (2 * B * H * L,), torch.float32)):
        n = math.prod(shape)
        m[name + "_buf"] = _guarded(n, t)
        m[name] = m[name + "_buf"][G:G + n].view(shape)
    return m


def _heads(c, m):
    """(b, h, n_b, Q, K, V) in float64 per (batch, head)."""
    D = c["H"] * DK
    x = m["qkv"].double()
    for b, n in enumerate(key_counts(c)):
        for h in range(c["H"]):
            yield (b, h, n) + tuple(x[b, :, i * D + h * DK:i * D + (h + 1) * DK] for i in range(3))


def _probs(Q, K, n):
    """S, P, lse, Delta, sum p Delta, R of one head with n keys (float64)."""
    L = Q.shape[0]
    scale = 1.0 / DK ** 0.5
    S = scale * Q @ K.T
    if n == 0:
        z = torch.zeros(L, L, dtype=torch.float64)
        return S, z, torch.full((L,), math.inf, dtype=torch.float64), z, torch.zeros(L, dtype=torch.float64), 0.0
    Sv = S[:, :n]
    lse = torch.logsumexp(Sv, dim=1)
    P = torch.zeros_like(S)
    P[:, :n] = torch.exp(Sv - lse[:, None])
    spread = Sv.max(dim=1).values - Sv.min(dim=1).values
    n_t = (n + KT - 1) // KT
    Delta = torch.zeros_like(S)
    Delta[:, :n] = (2 * (DK + 8) * F * scale * (Q.abs() @ K.abs().T))[:, :n] + \
        ((2 * spread + 4 * (n_t + 1)) * 2 * F)[:, None]
    spd = (P * Delta).sum(dim=1)
    assert float((Delta.max(dim=1).values + spd).max()) <= 0.5, "the linearisation of the bar does not hold"
    R = 2 * (n + 64) * F + 3 * F * math.log(max(n, 2)) + F * lse.abs()
    return S, P, lse, Delta, spd, R


def reference_fwd(c, m):
    """float64 out (B, L, D) and lse (B, H, L) with their bars; o_in / lse_in are the two rounded to the
    dtypes a backward kernel is handed."""
    B, L, H = c["B"], c["L"], c["H"]
    u, bf = U[c["dt"]], c["dt"] == "bf16"
    out, bar = torch.zeros(B, L, H * DK, dtype=torch.float64), torch.zeros(B, L, H * DK, dtype=torch.float64)
    lse, bar_lse = torch.zeros(B, H, L, dtype=torch.float64), torch.zeros(B, H, L, dtype=torch.float64)
    for b, h, n, Q, K, V in _heads(c, m):
        S, P, ls, Delta, spd, R = _probs(Q, K, n)
        Va = V.abs().clone()
        Vv = V.clone()
        Va[n:] = 0  # P is exactly 0 there (0 x the poison stays 0)
        Vv[n:] = 0
        A = P @ Va
        o = P @ Vv
        e = 1.5 * ((P * Delta) @ Va + spd[:, None] * A) + 4 * (n + 64) * F * A + (3 * F + u) * o.abs()
        if bf:
            e = e + u * A
        sl = slice(h * DK, (h + 1) * DK)
        out[b, :, sl], bar[b, :, sl] = o, e
        lse[b, h], bar_lse[b, h] = ls, 1.5 * spd + R
    return dict(out=out, bar_out=bar, lse=lse, bar_lse=bar_lse, o_in=out.to(DT[c["dt"]]), lse_in=lse.float())


def reference_bwd(c, m, o_in):
    """float64 dqkv (B, L, 3D) = [dQ | dK | dV] from (qkv, o_in, dout), its bar, and mag: the same sums on
    absolute values (what a row's norm is compared with to call it non-zero)."""
    B, L, H = c["B"], c["L"], c["H"]
    D = H * DK
    u, bf = U[c["dt"]], c["dt"] == "bf16"
    scale = 1.0 / DK ** 0.5
    ref, bar, mag = (torch.zeros(B, L, 3 * D, dtype=torch.float64) for _ in range(3))
    do_all, o_all = m["dout"].double(), o_in.double()
    for b, h, n, Q, K, V in _heads(c, m):
        sl = slice(h * DK, (h + 1) * DK)
        dO, O = do_all[b, :, sl], o_all[b, :, sl]
        S, P, ls, Delta, spd, R = _probs(Q, K, n)
        if n == 0:
            continue  # reference, bar and mag stay 0
        K, V = K.clone(), V.clone()
        K[n:] = 0  # P and dS are exactly 0 there
        V[n:] = 0
        eps = 1.5 * (Delta + spd[:, None]) + (R + 2 * F * ls.abs())[:, None] + 2 * F * S.abs()
        Dr = (dO * O).sum(dim=1)
        dP = dO @ V.T
        dS = P * (dP - Dr[:, None])
        e = P * (eps * (dP - Dr[:, None]).abs() +
                 2 * (DK + 8) * F * (dO.abs() @ V.abs().T + (dO.abs() * O.abs()).sum(dim=1)[:, None]))
        pe = P * eps
        if bf:
            e = e + u * (dS.abs() + e)
            pe = pe + u * P
        dSm = P * (dP.abs() + Dr.abs()[:, None])
        acc = 2 * (L + 64) * F
        dq, dk, dv = scale * dS @ K, scale * dS.T @ Q, P.T @ dO
        parts = ((dq, scale * (e @ K.abs() + acc * dS.abs() @ K.abs()), scale * dSm @ K.abs()),
                 (dk, scale * (e.T @ Q.abs() + acc * dS.abs().T @ Q.abs()), scale * dSm.T @ Q.abs()),
                 (dv, pe.T @ dO.abs() + acc * P.T @ dO.abs(), P.T @ dO.abs()))
        for i, (r, e_r, m_r) in enumerate(parts):
            cs = slice(i * D + h * DK, i * D + (h + 1) * DK)
            ref[b, :, cs], bar[b, :, cs], mag[b, :, cs] = r, e_r + u * r.abs(), m_r
    return dict(dqkv=ref, bar=bar, mag=mag)


def _rows(t):
    """(..., n x 128) -> (..., n, 128): one row per (batch, position, [q | k | v], head)."""
    return t.reshape(t.shape[:-1] + (t.shape[-1] // DK, DK))


def _check_guard(c, m, name):
    buf = m[name + "_buf"]
    raw = buf.view(_INT[buf.dtype])
    bad = torch.cat([raw[:G], raw[-G:]]) != GUARD[buf.dtype]
    assert not bool(bad.any()), f"{c['name']}: {int(bad.sum())} guard elements of {name} written, first at " \
                                f"{int(bad.nonzero()[0])} of the {2 * G}"


def _check_values(c, what, got, ref, bar):
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin]), f"{c['name']}: {what} is not +inf where no key exists"
    assert bool(torch.isfinite(got[fin]).all()), f"{c['name']}: non-finite {what}"
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    ratio = float((err / bar.clamp_min(1e-300)).max())
    over = err > bar
    assert not bool(over.any()), f"{c['name']}: {int(over.sum())} of {over.numel()} elements of {what} over the " \
                                 f"bar (worst ratio {ratio:.3g}), first at {tuple(int(i) for i in over.nonzero()[0])}"
    return ratio


def _row_rel(got, ref, mag):
    """Worst rel-L2 over the rows of 128 whose reference is non-zero."""
    gr, rr = _rows(got), _rows(ref)
    rn = rr.norm(dim=-1)
    keep = rn > 2.0 ** -40 * _rows(mag).norm(dim=-1)
    if not bool(keep.any()):
        return 0.0
    return float(((gr - rr).norm(dim=-1)[keep] / rn[keep]).max())


def verify(c, m, ref, after=None):
    """The outputs in m against ref (reference_fwd's dict for a 'fwd' case, reference_bwd's for a 'bwd'
    case): every element of the view within the bar, everything outside bit-identical to the guard pattern,
    and the inputs (``after``: name -> the tensor as read back after the call, default m's own) bit-identical
    to what make drew.  On the flat draw the worst per-row rel-L2 is held to ROW_TOL as well.  Returns
    (worst error / bar, worst per-row rel-L2); raises AssertionError."""
    for name, t in (after or {}).items():
        assert t.dtype == m[name].dtype and torch.equal(t.cpu().view(_INT[t.dtype]), m[name].view(_INT[t.dtype])), \
            f"{c['name']}: the input {name} changed"
    if c["kind"] == "fwd":
        _check_guard(c, m, "out")
        _check_guard(c, m, "lse")
        got = m["out"].double()
        ratio = max(_check_values(c, "out", got, ref["out"], ref["bar_out"]),
                    _check_values(c, "lse", m["lse"].double(), ref["lse"], ref["bar_lse"]))
        rel = _row_rel(got, ref["out"], ref["out"].abs())
    else:
        _check_guard(c, m, "dqkv")
        _check_guard(c, m, "ws")
        got = m["dqkv"].double()
        ratio = _check_values(c, "dqkv", got, ref["dqkv"], ref["bar"])
        rel = _row_rel(got, ref["dqkv"], ref["mag"])
    print(f"{c['name']}: worst error/bar {ratio:.3e}, worst row rel-L2 {rel:.3e}")
    if c["draw"] == "flat":
        tol = ROW_TOL[c["kind"], c["dt"]]
        assert rel < tol, f"{c['name']}: worst row rel-L2 {rel:.3e} >= {tol}"
    return ratio, rel


# ------------------------------------------------------------------------------------- CPU emulation

# draws on which a mutation stays under the rounding the bar must admit: ramp_down gives the last keys a
# weight of e^-8 per tile below the first tile's (so a key more or less at the end, or alpha = 1 left out,
# changes nothing), and on either ramp a pad key of score 0 sits that far under the maximum
BLIND = {"extra_key": {"ramp_down"}, "drop_last_key": {"ramp_down"}, "no_rescale": {"ramp_down"},
         "zero_pad_keys": {"ramp_up", "ramp_down"}}


def applies(c, mutate):
    """Whether the mutation changes the result of the case by more than rounding."""
    L, ns = c["L"], key_counts(c)
    raw = [L] * c["B"] if c["lens"] is None else c["lens"]
    if c["draw"] in BLIND.get(mutate, ()):
        return False
    return {"extra_key": True, "drop_last_key": any(n > 0 for n in ns), "guard": True,
            "zero_pad_keys": L % KT != 0 and any(n >= L for n in raw),
            # alpha != 1 needs a later tile that raises a row's maximum
            "no_rescale": any(n > KT for n in ns),
            "row_swap": L >= 2 and any(n > 0 for n in ns), "head_swap": c["H"] >= 2 and any(n > 0 for n in ns),
            "no_D": any(n > 0 for n in ns), "padded_key_grad": any(0 < n < L for n in ns),
            "drop_last_query": L >= 2 and any(n > 0 for n in ns), "unscaled_dq": any(n > 1 for n in ns)}[mutate]


def _f32_heads(c, m):
    D = c["H"] * DK
    x = m["qkv"].float()
    raw = [c["L"]] * c["B"] if c["lens"] is None else c["lens"]
    for b, n in enumerate(key_counts(c)):
        for h in range(c["H"]):
            yield (b, h, n, raw[b]) + tuple(x[b, :, i * D + h * DK:i * D + (h + 1) * DK] for i in range(3))


def emulate_fwd(c, m, mutate=None):
    """The forward kernels' arithmetic, written into m['out'] and m['lse'].  ``mutate`` names a deliberate
    fault (FWD_MUTATIONS)."""
    L, bf = c["L"], c["dt"] == "bf16"
    scale = torch.tensor(1.0 / DK ** 0.5, dtype=torch.float32)
    Lp = KT * ((L + KT) // KT)  # whole tiles with at least one row past L, staged as zeros
    out = torch.zeros(c["B"], L, c["H"] * DK)
    lse = torch.zeros(c["B"], c["H"], L)
    for b, h, n, raw, Q, K, V in _f32_heads(c, m):
        Kp, Vp = torch.zeros(Lp, DK), torch.zeros(Lp, DK)
        Kp[:L], Vp[:L] = K, V
        admit = n
        if mutate == "extra_key":
            admit = n + 1
        elif mutate == "drop_last_key":
            admit = max(n - 1, 0)
        elif mutate == "zero_pad_keys" and raw >= L:
            admit = KT * ((L + KT - 1) // KT)
        S = (Q @ Kp.T) * scale
        S[:, admit:] = -math.inf
        m_run, l_run, O = torch.full((L,), -math.inf), torch.zeros(L), torch.zeros(L, DK)
        n_t = (admit + KT - 1) // KT
        for t in range(n_t):
            s = S[:, t * KT:(t + 1) * KT]
            m_new = torch.maximum(m_run, s.max(dim=1).values)
            alpha = torch.where(m_run == -math.inf, torch.zeros(L), torch.exp(m_run - m_new))
            p = torch.where(s == -math.inf, torch.zeros_like(s), torch.exp(s - m_new[:, None]))
            l_run = l_run * alpha + p.sum(dim=1)
            if not (mutate == "no_rescale" and t == n_t - 1 and t > 0):
                O = O * alpha[:, None]
            O = O + (p.bfloat16().float() if bf else p) @ Vp[t * KT:(t + 1) * KT]
            m_run = m_new
        has = l_run > 0
        inv = torch.where(has, 1.0 / l_run.clamp_min(1e-37), torch.zeros(L))
        out[b, :, h * DK:(h + 1) * DK] = O * inv[:, None]
        lse[b, h] = torch.where(has, m_run + torch.log(l_run.clamp_min(1e-37)), torch.full((L,), math.inf))
    if mutate == "row_swap":
        out[:, L - 1] = out[:, L - 2]
    if mutate == "head_swap":
        out = out.roll(DK, dims=2)
    m["out"].copy_(out.to(m["out"].dtype))
    m["lse"].copy_(lse)
    if mutate == "guard":
        m["out_buf"].view(_INT[m["out_buf"].dtype])[G + m["out"].numel()] += 1


def emulate_bwd(c, m, o_in, lse_in, mutate=None):
    """The backward kernels' arithmetic from (qkv, o_in, dout) and the fp32 row log-sum-exp, written into
    m['dqkv'].  ``mutate`` names a deliberate fault (BWD_MUTATIONS)."""
    L, H, bf = c["L"], c["H"], c["dt"] == "bf16"
    D = H * DK
    scale = torch.tensor(1.0 / DK ** 0.5, dtype=torch.float32)
    dqkv = torch.zeros(c["B"], L, 3 * D)
    do_all, o_all = m["dout"].float(), o_in.float()
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    for b, h, n, raw, Q, K, V in _f32_heads(c, m):
        sl = slice(h * DK, (h + 1) * DK)
        dO, O = do_all[b, :, sl], o_all[b, :, sl]
        admit = n + 1 if (mutate == "padded_key_grad" and 0 < n < L) else n
        S = (Q @ K.T) * scale
        P = torch.exp(S - lse_in[b, h][:, None])
        P[:, admit:] = 0
        Dr = torch.zeros(L) if mutate == "no_D" else (dO * O).sum(dim=1)
        dS = P * (dO @ V.T - Dr[:, None])
        Pr, dSr = rnd(P), rnd(dS)
        dq = dSr @ K if mutate == "unscaled_dq" else (dSr @ K) * scale
        if mutate == "drop_last_query":
            Pr, dSr = Pr.clone(), dSr.clone()
            Pr[L - 1] = 0
            dSr[L - 1] = 0
        dqkv[b, :, sl] = dq
        dqkv[b, :, D + h * DK:D + (h + 1) * DK] = (dSr.T @ Q) * scale
        dqkv[b, :, 2 * D + h * DK:2 * D + (h + 1) * DK] = Pr.T @ dO
    m["dqkv"].copy_(dqkv.to(m["dqkv"].dtype))
    if mutate == "guard":
        m["dqkv_buf"].view(_INT[m["dqkv_buf"].dtype])[G - 1] += 1
