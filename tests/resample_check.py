"""Yardstick of the sample-rate conversion (vo_resample, ``ops.resample``), written from the
rule in plain numpy float64 without looking at the package (the resampling twin of tests/pcm_check.py).

The rule.  Z = 64 zero crossings, ROLLOFF = 0.9475937167399596, BETA = 14.769656459379492.  With g = gcd(sr_in,
sr_out), O = sr_in / g, M = sr_out / g: c = min(O, M) ROLLOFF / O, W = ceil(Z / c), T = 2 W + 1.  Coefficients, for
r in [0, M) and j in [0, T): t = c (j - W - r / M), h[r][j] = c sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA) for
|t| < Z, else 0.  Output n of a row x of n_b samples (0 outside): q = (n O) div M, r = (n O) mod M,
res[n] = sum_j h[r][j] x[q - W + j]; L_b = ceil(n_b M / O).  A call drops ``skip`` outputs from the front (clamped to
[0, L_b]) and writes m_b = clamp(L_b - skip, 0, N_out) of them, then zeros up to N_out.

``model`` evaluates a row in float64 over the fp32 input values as the kernel reads them and returns, per output,
y64 = sum h64 x, S = sum |h64| |x| and m_b.  ``check`` asserts, per element,
  * |y - y64| <= (T + 2) 2^-24 1.001 S.  Derived, not measured: one rounding of each coefficient to fp32 (2^-24 of
    its term), at most T roundings of the fp32 dot product in any order, with or without FMA (each at most 2^-24 of
    a partial sum that S bounds), one spare, and 1.001 for the second-order terms;
  * y == 0 exactly where S == 0;
  * y == 0 for i >= m_b;
and ``check_guard`` that the GUARD elements behind a ``guarded`` buffer still hold their poison.

``emulate`` is the conversion in fp32 numpy with one deliberate fault of MUTATIONS, for the checker's self-test
(tests/test_resample_cpu.py).  ``matrix`` / ``impulses`` build the inputs the CPU self-test and the GPU tests share.
"""

import math

import numpy as np

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
GUARD = 64
POISON_I16 = 0x5A5A
MUTATIONS = ("phase_plus_one", "centre_off_by_one", "skip_ignored", "tail_not_zeroed", "len_floor",
             "last_tap_dropped")
RATIOS = ((2, 1), (1, 2), (3, 2), (2, 3), (7, 5), (5, 7))
IMPULSE = 0.75


def geometry(sr_in, sr_out):
    """(O, M, W, T) of two rates."""
    g = math.gcd(sr_in, sr_out)
    O, M = sr_in // g, sr_out // g
    c = min(O, M) * ROLLOFF / O
    W = int(math.ceil(Z / c))
    return O, M, W, 2 * W + 1


def table64(O, M):
    """The (M, T) coefficients in float64, unrounded."""
    _, _, W, T = geometry(O, M)
    c = min(O, M) * ROLLOFF / O
    r = np.arange(M, dtype=np.float64)[:, None]
    j = np.arange(T, dtype=np.float64)[None, :]
    t = c * (j - W - r / M)
    inside = np.abs(t) < Z
    u = np.where(inside, t / Z, 0.0)
    h = c * np.sinc(t) * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA)
    return np.where(inside, h, 0.0)


def length(n, O, M):
    return -((-int(n) * M) // O)


def as_read(x, max_wav_value=32768.0):
    """The fp32 values the kernel reads: an fp32 array as it is, an int16 s as float32(s) / float32(max_wav_value)."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) / np.float32(max_wav_value)
    assert x.dtype == np.float32, x.dtype
    return x


def _windows(x, n_b, n, O, M, W, T, first=0):
    """(r, xw): the table row of every output index in ``n`` and its T input samples x[q - W + first + j], zero
    outside [0, n_b).  Only x[:n_b] is read."""
    n = np.asarray(n, np.int64)
    q, r = (n * O) // M, (n * O) % M
    xp = np.zeros(n_b + 2 * W + 2, np.asarray(x).dtype)
    xp[W:W + n_b] = x[:n_b]
    idx = q[:, None] + first + np.arange(T)[None, :]
    return r, xp[np.clip(idx, 0, xp.size - 1)]


def model(x, n_b, skip, O, M, N_out, h64=None):
    """One row: x the fp32 values as read (at least n_b of them), -> (y64 (N_out,), S (N_out,), m_b)."""
    _, _, W, T = geometry(O, M)
    h64 = table64(O, M) if h64 is None else h64
    n_b = int(n_b)
    L = length(n_b, O, M)
    s = min(max(int(skip), 0), L)
    m = min(max(L - s, 0), N_out)
    y64, S = np.zeros(N_out), np.zeros(N_out)
    if m:
        r, xw = _windows(np.asarray(x, np.float32).astype(np.float64), n_b, s + np.arange(m), O, M, W, T)
        y64[:m] = (h64[r] * xw).sum(axis=1)
        S[:m] = (np.abs(h64[r]) * np.abs(xw)).sum(axis=1)
    return y64, S, m


def check(y, y64, S, m_b, T, name="resample"):
    """``y``: one fp32 output row (N_out,), against ``model``'s row."""
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape == y64.shape, f"{name}: result is {y.dtype} {y.shape}"
    past = np.flatnonzero(y[m_b:] != 0)  # NaN != 0: an unwritten (poisoned) element is caught too
    assert past.size == 0, f"{name}: output {m_b + int(past[0])} past the row's {m_b} samples is {y[m_b + past[0]]!r}"
    assert not np.isnan(y[:m_b]).any(), f"{name}: NaN at output {int(np.flatnonzero(np.isnan(y[:m_b]))[0])}"
    zero = np.flatnonzero((S == 0) & (y != 0))
    assert zero.size == 0, f"{name}: output {int(zero[0])} reads only zeros but is {y[zero[0]]!r}"
    err = np.abs(y.astype(np.float64) - y64)
    tol = (T + 2) * 2.0 ** -24 * 1.001 * S
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, (f"{name}: output {int(bad[0])} is {y[bad[0]]!r}, float64 gives {y64[bad[0]]!r}: error "
                           f"{err[bad[0]]:.3e} > {tol[bad[0]]:.3e}")
    return float((err[:m_b] / np.maximum(tol[:m_b], 1e-300)).max()) if m_b else 0.0


def guarded(B, N_out, dtype):
    """A flat buffer of B * N_out + GUARD poisoned elements (NaN, or 0x5A5A for int16): a call writes the first
    B * N_out."""
    return np.full(B * N_out + GUARD, POISON_I16 if np.dtype(dtype) == np.int16 else np.nan, dtype)


def split_guard(buf, B, N_out):
    buf = np.asarray(buf)
    assert buf.shape == (B * N_out + GUARD,), buf.shape
    return buf[:B * N_out].reshape(B, N_out), buf[B * N_out:]


def check_guard(buf, B, N_out, name="resample"):
    g = split_guard(buf, B, N_out)[1]
    ok = (g == POISON_I16) if g.dtype == np.int16 else np.isnan(g)
    assert ok.all(), f"{name}: guard element {int(np.flatnonzero(~ok)[0])} behind the buffer was written"


def untouched(buf):
    """True when every element of a poisoned buffer still holds its poison (a refused call)."""
    buf = np.asarray(buf)
    return bool(((buf == POISON_I16) if buf.dtype == np.int16 else np.isnan(buf)).all())


def emulate(x, n_b, skip, O, M, N_out, mutation=None, h32=None):
    """One row in fp32 numpy (products and sum in fp32) with one fault of MUTATIONS (None: none) -> (y (N_out,)
    fp32, m_b as the faulty code would report it)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    _, _, W, T = geometry(O, M)
    h32 = table64(O, M).astype(np.float32) if h32 is None else h32
    n_b = int(n_b)
    L = (n_b * M) // O if mutation == "len_floor" else length(n_b, O, M)
    s = 0 if mutation == "skip_ignored" else min(max(int(skip), 0), L)
    m = min(max(L - s, 0), N_out)
    y = np.zeros(N_out, np.float32)
    if m:
        r, xw = _windows(np.asarray(x, np.float32), n_b, s + np.arange(m), O, M, W, T,
                         first=1 if mutation == "centre_off_by_one" else 0)
        if mutation == "phase_plus_one":
            r = (r + 1) % M
        h = h32[r]
        if mutation == "last_tap_dropped":
            h = h.copy()
            h[:, T - 1] = 0
        y[:m] = (h * xw).sum(axis=1, dtype=np.float32)
    if mutation == "tail_not_zeroed" and m < N_out:
        y[m:] = np.float32(1e-3)
    return y, m


# ---------------------------------------------------------------------------------- shared inputs

def row_lengths(O, M, tile):
    """The row lengths of a ratio's case matrix: 0, 1, 2; W, W + 1, 2 W + 1; the n_b whose L_b is tile - 1, tile,
    tile + 1 and 2 tile + 1 (the smallest n_b with L_b at least that, where M > O skips it); the first n_b past
    2 W + 1 with n_b M mod O equal to 0, 1 and O - 1."""
    _, _, W, _ = geometry(O, M)
    ns = [0, 1, 2, W, W + 1, 2 * W + 1]
    for want in (tile - 1, tile, tile + 1, 2 * tile + 1):
        n = (want * O) // M
        while length(n, O, M) < want:
            n += 1
        while n > 0 and length(n - 1, O, M) >= want:
            n -= 1
        ns.append(n)
    for rem in sorted({0, 1 % O, O - 1}):
        n = 2 * W + 2
        while (n * M) % O != rem:
            n += 1
        ns.append(n)
    return ns


def noise_batch(lens, kind, seed, extra=5):
    """(x (B, max + extra), lens): seeded uniform noise in [-0.5, 0.5] (int16: [-16384, 16384]) in each row's first
    lens[b] elements; behind them NaN (int16: 0x7FFF), which a correct call never reads."""
    rng = np.random.default_rng(seed)
    N = max(lens) + extra
    if kind == "int16":
        x = np.full((len(lens), N), 0x7FFF, np.int16)
        for b, n in enumerate(lens):
            x[b, :n] = rng.integers(-16384, 16385, n).astype(np.int16)
    else:
        x = np.full((len(lens), N), np.nan, np.float32)
        for b, n in enumerate(lens):
            x[b, :n] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    return x, list(lens)


def impulse_rows(O, M):
    """(x (3, n_b + 5) fp32, n_b, ks): rows of n_b = 4 W + 7 samples, zero except IMPULSE at k = 0, n_b - 1 and
    one interior k; NaN behind the rows."""
    _, _, W, _ = geometry(O, M)
    n_b = 4 * W + 7
    ks = [0, n_b - 1, 2 * W + 3]
    x = np.full((3, n_b + 5), np.nan, np.float32)
    x[:, :n_b] = 0
    for b, k in enumerate(ks):
        x[b, k] = IMPULSE
    return x, n_b, ks


def impulse_expected(h32, k, n_b, O, M, N_out):
    """Bit for bit what an impulse row gives: float32(h32[r][j]) * float32(IMPULSE) at j = k - q + W where that is a
    tap, exactly 0 elsewhere."""
    _, _, W, T = geometry(O, M)
    m = min(length(n_b, O, M), N_out)
    n = np.arange(m, dtype=np.int64)
    q, r = (n * O) // M, (n * O) % M
    j = k - q + W
    ok = (j >= 0) & (j < T)
    y = np.zeros(N_out, np.float32)
    y[:m][ok] = h32[r[ok], j[ok]] * np.float32(IMPULSE)
    return y
