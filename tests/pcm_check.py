"""Checker of a 16-bit PCM waveform written on the device (vo_conv_post_pcm16, ``Generator.run(pcm_scale=...)``)
against an fp32 reference waveform (the PCM twin of tests/attn_check.py).

The store under test is q = (int16) clamp(trunc(y * scale), -32768, 32767), the product formed in fp32, truncated
toward zero, NaN -> 0 (include/vonoma.h).  ``expected_pcm`` is that expression in numpy fp32.

``check_pcm(q, y_ref, scale, rows)`` asserts
  * |q - expected| <= 1 everywhere;
  * q == expected wherever y_ref * scale is at least BAND = 0.01 away from an integer.  y_ref comes from another
    compilation of the same fp32 expression (the fp32 instantiation of the kernel, or an eager run): the two may
    differ in the last bit of y, |dy| <= 2^-24 |y| <= 6e-8, which scaled by 32768 stays below 0.003 -- so only a
    product within 0.003 of an integer can truncate to the neighbouring integer, and BAND leaves a factor 3;
  * q == 0 past rows[b] (ragged batches);
  * the GUARD elements after the buffer still hold GUARD_VALUE (when ``q`` is the guarded flat buffer of ``guarded``).
The excluded band is a condition, not a tolerance: the check itself asserts that at most BAND_CAP = 5 % of the
compared samples fall in it (uniform fractional parts give 2 %), so a reference that sits on integers -- silence, a
saturated waveform -- cannot pass by exclusion.  Saturated and NaN stores are therefore asserted by equality with
``expected_pcm`` where they are tested, not through the band.

``emulate`` is the store on the CPU with one deliberate fault (MUTATIONS), for the checker's self-test.
"""

import numpy as np

GUARD = 64
GUARD_VALUE = 0x5A5A
BAND = 0.01
BAND_CAP = 0.05
MUTATIONS = ("round_nearest", "wrap", "tail_sample", "row_shift", "guard")


def expected_pcm(y, scale):
    """clip(trunc(y * scale), -32768, 32767) with the product in fp32 and NaN -> 0, as int16."""
    p = np.asarray(y, np.float32) * np.float32(scale)
    assert p.dtype == np.float32
    with np.errstate(invalid="ignore"):
        q = np.clip(np.trunc(p), -32768.0, 32767.0)
    return np.where(np.isnan(p), np.float32(0), q).astype(np.int16)


def in_band(y, scale):
    """True where the fp32 product y * scale is less than BAND away from an integer (NaN: False)."""
    p = (np.asarray(y, np.float32) * np.float32(scale)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(p - np.rint(p)) < BAND


def guarded(B, T):
    """A flat int16 buffer of B * T + GUARD elements, every one GUARD_VALUE: a kernel writes the first B * T."""
    return np.full(B * T + GUARD, GUARD_VALUE, np.int16)


def split_guard(buf, B, T):
    buf = np.asarray(buf)
    assert buf.dtype == np.int16 and buf.shape == (B * T + GUARD,), (buf.dtype, buf.shape)
    return buf[:B * T].reshape(B, T), buf[B * T:]


def check_guard(buf, B, T, name="pcm"):
    _, g = split_guard(buf, B, T)
    bad = np.flatnonzero(g != GUARD_VALUE)
    assert bad.size == 0, f"{name}: guard element {int(bad[0])} after the buffer changed to {int(g[bad[0]])}"


def check_pcm(q, y_ref, scale, rows=None, name="pcm"):
    """``q``: the int16 result, (B, T) or the guarded flat buffer (``guarded``); ``y_ref`` (B, T) fp32;
    ``rows``: per-utterance valid sample counts (None: all T).  Returns the fraction of compared samples in the
    band."""
    y_ref = np.asarray(y_ref)
    assert y_ref.dtype == np.float32 and y_ref.ndim == 2, (y_ref.dtype, y_ref.shape)
    B, T = y_ref.shape
    q = np.asarray(q)
    if q.ndim == 1:
        check_guard(q, B, T, name)
        q = split_guard(q, B, T)[0]
    assert q.dtype == np.int16 and q.shape == (B, T), f"{name}: result is {q.dtype} {q.shape}, want int16 {(B, T)}"
    rows = [T] * B if rows is None else [min(max(int(r), 0), T) for r in rows]
    valid = np.arange(T)[None, :] < np.asarray(rows)[:, None]
    past = q[~valid]
    assert not past.any(), f"{name}: {int(np.count_nonzero(past))} non-zero samples past the utterances' ends"
    if not valid.any():
        return 0.0
    want = expected_pcm(y_ref, scale)
    diff = np.abs(q.astype(np.int32) - want.astype(np.int32))
    worst = np.unravel_index(np.argmax(np.where(valid, diff, 0)), diff.shape)
    assert diff[valid].max() <= 1, (f"{name}: sample {worst} is {int(q[worst])}, expected {int(want[worst])} "
                                    f"(y = {float(y_ref[worst])!r})")
    band = in_band(y_ref, scale) & valid
    frac = float(band.sum()) / float(valid.sum())
    assert frac <= BAND_CAP, f"{name}: {frac:.1%} of the samples lie within {BAND} of an integer (cap {BAND_CAP:.0%})"
    exact = valid & ~band
    bad = exact & (diff != 0)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{name}: {int(bad.sum())} samples off by one outside the band, first at {i}: "
                             f"{int(q[i])} for y * scale = {float(np.float32(y_ref[i]) * np.float32(scale))!r}")
    return frac


def emulate(y, scale, rows=None, mutate=None):
    """The store on the CPU into a guarded buffer, with one fault of MUTATIONS (None: none)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    y = np.asarray(y, np.float32)
    B, T = y.shape
    rows = [T] * B if rows is None else [min(max(int(r), 0), T) for r in rows]
    p = y * np.float32(scale)
    with np.errstate(invalid="ignore"):
        if mutate == "round_nearest":
            q = np.clip(np.rint(p), -32768.0, 32767.0)
        elif mutate == "wrap":  # the host cast past the range: modulo 2^16
            q = ((np.trunc(np.nan_to_num(p)).astype(np.int64) + 32768) % 65536 - 32768).astype(np.float32)
        else:
            q = np.clip(np.trunc(p), -32768.0, 32767.0)
    q = np.where(np.isnan(p), np.float32(0), q).astype(np.int16)
    for b, r in enumerate(rows):
        q[b, r:] = 0
    if mutate == "row_shift":
        q = np.roll(q, 1, axis=0)
    if mutate == "tail_sample":
        b = next(b for b, r in enumerate(rows) if r < T)
        q[b, T - 1] = 1
    buf = guarded(B, T)
    buf[:B * T] = q.reshape(-1)
    if mutate == "guard":
        buf[B * T + GUARD - 1] = 0
    return buf


# ---------------------------------------------------------------------------------- conv_post operands

def post_case(dt, C, K, T, B=3):
    return dict(name=f"{dt}-C{C}-K{K}-T{T}", dt=dt, C=C, K=K, T=T, B=B)


def post_operands(c, seed=0):
    """x (B, T, C) fp32 (bf16 values when the case is bf16), w (K, C) fp32 and the bias of a conv_post call whose
    pre-tanh sums spread over about [-2, 2]: the waveform fills the int16 range and its fractional parts are
    spread evenly (band fraction 2 %)."""
    import torch
    g = torch.Generator().manual_seed(7000 + seed + 31 * c["T"] + c["C"] + c["K"])
    x = torch.randn(c["B"], c["T"], c["C"], generator=g)
    if c["dt"] == "bf16":
        x = x.bfloat16().float()
    w = torch.randn(c["K"], c["C"], generator=g) * (1.6 / (c["K"] * c["C"]) ** 0.5)
    return x, w, 0.05


def post_reference(x, w, bias, slope=0.01, rows=None):
    """tanh(conv(lrelu(x))) of utterance b's first rows[b] rows alone, in float64 rounded to fp32; 0 past them."""
    import torch
    B, T, C = x.shape
    K = w.shape[0]
    y = torch.zeros(B, T, dtype=torch.float32)
    for b in range(B):
        r = T if rows is None else min(max(int(rows[b]), 0), T)
        if r == 0:
            continue
        xb = torch.nn.functional.leaky_relu(x[b, :r].double(), slope).T[None]
        y[b, :r] = torch.tanh(torch.nn.functional.conv1d(xb, w.double().T[None], padding=(K - 1) // 2)[0, 0]
                              + bias).float()
    return y
