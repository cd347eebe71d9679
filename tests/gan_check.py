"""Checker of the GAN loss-term kernels (vo_gan_reduce / _grad and their _multi forms) against arithmetic done
elsewhere: float64 sums with a derived bar, gradients against the same fp32 expression evaluated by torch on the
CPU, guard bands, NaN padding, and a second run that must repeat the first bit for bit.

A case is a dtype and a list of terms (``case``, ``term``).  ``make`` draws the operands on the CPU: every operand
is a (rows, width) view with leading dimension ld at element offset ``off`` of a NaN-filled buffer, so the padding
columns and the elements before and after the view are NaN.  ``run`` drives a backend (the GPU test's ``ops``
wrapper, or in the CPU self-test ``Standin``) through the four entry points, twice, and ``verify`` checks, naming
the first that fails: guards, operands, gradients, sums, the accumulate rule, the ``ops`` wrapper of the multi
entry, determinism.

Term element (x of a, y of b):   0: |x - y|     1: (1 - x)^2     2: x^2
Gradient of scale * sum wrt x:   0: scale * sign(x - y) (0 at a tie)     1: -2 (1 - x) scale     2: 2 x scale

Gradient: every element equals, bit for bit, that fp32 expression evaluated by torch on the CPU and rounded to
the tensor's dtype (no product feeds a sum there, so there is nothing a compiler could fuse; the factor 2 is
exact, so the order of the two multiplies does not matter).

Sum: |got - S| <= (k + 4) 2^-24 S, S the float64 sum of the float64 term values (all values are >= 0, so S is
also the sum of magnitudes) and k the longest chain of fp32 additions a value passes through.  With u units of V
elements (V = 8 where the term's rows allow 8-element vectors, else 1) the reduction runs g = min(ceil(u / 256),
512) blocks of 256 threads (the grid rule of gan_multi_args in csrc/disc.hip), and a value is added
    V ceil(u / (256 g))  times in its thread's accumulator (one unit per trip, V elements each),
    6                    in the wave's butterfly,
    3                    across the block's four waves,
    ceil(g / 64) + 6     in the final kernel (a lane's strided partials, then its wave's butterfly).
Each addition loses at most 2^-24 of the running sum, which never exceeds S (1 + small), so k additions lose
<= k 2^-24 S to first order.  The 4 covers the at most three roundings inside a value (the difference, the
product -- fused into the add or not -- and the conversion) and the multiply by the term's scale.
Sensitivity: values of ordinary elements lie in [VMIN, VMAX], so one dropped or doubled unit moves the sum by at
least V VMIN while the bar is at most (k + 4) 2^-24 n VMAX; ``case`` asserts that the ratio is >= FACTOR.  At
n > 2^20 elements no spread of values can keep that ratio above 1 (it is at most 2^24 V / ((k + 4) n)): the two
cases just above 4096 * 256 units, which exist for the gradient's grid cap, are marked ``grad_cap`` and exempt;
a unit dropped there shows in the gradient, which is compared bit for bit.

Accumulate: vo_gan_reduce into out = ACC0 gives fp32(ACC0 + s), s what it gives into out = 0.  The multi entry
overwrites: its output slots start as the guard pattern.
"""

import math

import torch

GAN_L1, GAN_ONE_MINUS_SQ, GAN_SQ = 0, 1, 2
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
GUARD = 0x5A5AA5A5          # a fixed bit pattern (a finite fp32, about 1.5e16; two finite bf16)
GUARD_N = 64                # guard elements on each side of a gradient buffer and of the output vector
WS_GUARD_N = 256            # guard floats after the queried workspace
VMIN, VMAX = 0.85, 1.15     # term values of ordinary elements
FACTOR = 2.0                # a dropped / doubled unit against the sum bar, at least
ACC0 = 3.25
FAILURES = ("guard", "operand", "gradient", "sum bar", "accumulate", "multi", "determinism")


def term(kind, rows, width, *, lda=None, ldb=None, off=0, scale=1.0, special=False):
    """One term.  lda / ldb: leading dimensions (None = width); off: a's offset in elements from its 16-byte
    aligned buffer; special: a few elements with value 0 (a tie a == b, a == 1, a == 0 for kind 0, 1, 2)."""
    lda = width if lda is None else lda
    ldb = width if ldb is None else ldb
    assert kind in (0, 1, 2) and rows >= 1 and width >= 1 and lda >= width and ldb >= width
    return dict(kind=kind, rows=rows, width=width, lda=lda, ldb=ldb, off=off, scale=float(scale), special=special)


def vec8(c, t):
    """The v8 predicate of gan_multi_args: width and leading dimensions multiples of 8, bases 16-byte aligned
    (b and the gradient start aligned here)."""
    isz = 2 if c["dt"] == "bf16" else 4
    return (t["width"] % 8 == 0 and t["lda"] % 8 == 0 and (t["off"] * isz) % 16 == 0 and
            (t["kind"] != 0 or t["ldb"] % 8 == 0))


def chain(c, t):
    """(V, units, k): the longest chain of fp32 additions of the term's reduction (module docstring)."""
    V = 8 if vec8(c, t) else 1
    u = t["rows"] * t["width"] // V
    g = min((u + 255) // 256, 512)
    return V, u, V * math.ceil(u / (256 * g)) + 6 + 3 + math.ceil(g / 64) + 6


def case(name, dt, terms, *, grad_cap=False):
    c = dict(name=f"{dt}_{name}", dt=dt, terms=list(terms), grad_cap=grad_cap,
             seed=(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 31 + len(dt)) % (2 ** 31))
    for t in c["terms"]:
        V, u, k = chain(c, t)
        ratio = V * VMIN * 2.0 ** 24 / ((k + 4) * t["rows"] * t["width"] * VMAX)
        assert grad_cap or ratio >= FACTOR, f"{c['name']}: a dropped unit would sit at {ratio:.2f} of the sum bar"
        assert not grad_cap or u > 4096 * 256
        assert not t["special"] or t["rows"] * t["width"] // V >= 4, "specials leave the last unit ordinary"
    return c


def _pattern(n, dtype=torch.float32):
    words = n if dtype == torch.float32 else (n + 1) // 2
    return torch.full((words,), GUARD, dtype=torch.int32).view(dtype)[:n].clone()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def view(buf, t, which="a"):
    """The (rows, width) operand view of a term inside its buffer (any device)."""
    ld, off = (t["lda"], t["off"]) if which == "a" else (t["ldb"], 0)
    return buf.as_strided((t["rows"], t["width"]), (ld, 1), off)


def _operand(n, kind, dtype, g):
    """(a, b) of n ordinary elements, exact in dtype, whose term values lie in [VMIN, VMAX]: the generating
    magnitude is in [0.95, 1.05] and rounding a to bf16 moves it by at most 2.1 * 2^-8."""
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    mag = 0.95 + 0.1 * torch.rand(n, generator=g)
    if kind == 0:
        b = (2 * torch.rand(n, generator=g) - 1).to(dtype)
        return (b.float() + sign * mag).to(dtype), b
    return ((1.0 + sign * mag) if kind == 1 else sign * mag).to(dtype), None


def fresh_out(c, ws_floats):
    dtype, n = TDT[c["dt"]], len(c["terms"])
    grads = lambda: [_pattern(t["rows"] * t["width"] + 2 * GUARD_N, dtype) for t in c["terms"]]
    single = _pattern(n + 2 * GUARD_N)
    single[GUARD_N:GUARD_N + n] = 0.0  # vo_gan_reduce adds into its output
    acc = _pattern(n + 2 * GUARD_N)
    acc[GUARD_N:GUARD_N + n] = ACC0
    return dict(sum_single=single, sum_acc=acc, sum_multi=_pattern(n + 2 * GUARD_N), sum_ops=None,
                g_single=grads(), g_multi=grads(),
                ws_buf=torch.cat([torch.full((ws_floats,), float("nan")), _pattern(WS_GUARD_N)]))


def make(c, ws_floats=None):
    """CPU buffers of the case: per term a_buf / b_buf (NaN outside the views), and two output sets.  ws_floats:
    floats of the multi entry's workspace (None = vo_gan_reduce_multi_workspace_size(n), from the library)."""
    if ws_floats is None:
        from visual_onoma_to_wave_amd import _lib
        ws_floats = int(_lib.lib().vo_gan_reduce_multi_workspace_size(len(c["terms"]))) // 4
    g = torch.Generator().manual_seed(c["seed"])
    dtype = TDT[c["dt"]]
    m = dict(a_buf=[], b_buf=[], ws_floats=ws_floats)
    for t in c["terms"]:
        n = t["rows"] * t["width"]
        a, b = _operand(n, t["kind"], dtype, g)
        if t["special"]:  # value 0 at elements 0, 9 and 18 (never the last unit): a tie, a == 1, a == 0
            for i in (0, 9, 18):
                if i < n - 8:
                    a[i] = b[i] if t["kind"] == 0 else (1.0 if t["kind"] == 1 else 0.0)
        ab = torch.full((t["off"] + t["rows"] * t["lda"] + 8,), float("nan"), dtype=dtype)
        view(ab, t).copy_(a.view(t["rows"], t["width"]))
        m["a_buf"].append(ab)
        bb = None
        if b is not None:
            bb = torch.full((t["rows"] * t["ldb"] + 8,), float("nan"), dtype=dtype)
            view(bb, t, "b").copy_(b.view(t["rows"], t["width"]))
        m["b_buf"].append(bb)
    m["a_orig"] = [x.clone() for x in m["a_buf"]]
    m["b_orig"] = [None if x is None else x.clone() for x in m["b_buf"]]
    m["outs"] = [fresh_out(c, ws_floats), fresh_out(c, ws_floats)]
    return m


def values(kind, x, y):
    """Term values in the dtype of x (float64 for the reference, fp32 for the stand-in)."""
    return (x - y).abs() if kind == 0 else ((1 - x) * (1 - x) if kind == 1 else x * x)


def grad32(kind, x, y, s):
    """The gradient expression in fp32 on the CPU (x, y fp32 tensors, s an fp32 scalar tensor)."""
    if kind == 0:
        d = x - y
        zero = torch.zeros((), dtype=torch.float32)
        return torch.where(d > 0, s, torch.where(d < 0, -s, zero)).expand_as(x)
    return (-2.0 * (1.0 - x)) * s if kind == 1 else (2.0 * x) * s


def reference(c, m):
    """Per term: S (float64 sum), bar, and the gradient in the tensor's dtype."""
    ref = dict(S=[], bar=[], grad=[])
    for i, t in enumerate(c["terms"]):
        a = view(m["a_orig"][i], t)
        b = view(m["b_orig"][i], t, "b") if t["kind"] == 0 else None
        S = float(values(t["kind"], a.double(), None if b is None else b.double()).sum())
        ref["S"].append(S)
        ref["bar"].append((chain(c, t)[2] + 4) * 2.0 ** -24 * S)
        s = torch.tensor(t["scale"], dtype=torch.float32)
        ref["grad"].append(grad32(t["kind"], a.float(), None if b is None else b.float(), s).to(TDT[c["dt"]]))
    return ref


def run(c, m, be, dev=None):
    """Both runs of the case through the backend ``be`` (gan_reduce, gan_reduce_grad, gan_reduce_multi,
    gan_reduce_grad_multi as in ops, and gan_reduce_multi_into(kinds, As, Bs, scale, out, ws) with the caller's
    output vector and workspace).  dev: the device the buffers are moved to and back from."""
    to = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    terms = c["terms"]
    n = len(terms)
    kinds = [t["kind"] for t in terms]
    a_buf = [to(x) for x in m["a_buf"]]
    b_buf = [None if x is None else to(x) for x in m["b_buf"]]
    As = [view(a_buf[i], t) for i, t in enumerate(terms)]
    Bs = [view(b_buf[i], t, "b") if t["kind"] == 0 else None for i, t in enumerate(terms)]
    scale = to(torch.tensor([t["scale"] for t in terms], dtype=torch.float32))
    inner = lambda buf, k: buf[GUARD_N:GUARD_N + k]
    for o in m["outs"]:
        d = {k: to(o[k]) for k in ("sum_single", "sum_acc", "sum_multi", "ws_buf")}
        gs, gm = [to(x) for x in o["g_single"]], [to(x) for x in o["g_multi"]]
        for i, t in enumerate(terms):
            be.gan_reduce(kinds[i], As[i], Bs[i], out=inner(d["sum_single"], n)[i])
            be.gan_reduce(kinds[i], As[i], Bs[i], out=inner(d["sum_acc"], n)[i])
            be.gan_reduce_grad(kinds[i], As[i], Bs[i], scale[i], out=inner(gs[i], t["rows"] * t["width"]))
        be.gan_reduce_multi_into(kinds, As, Bs, scale, inner(d["sum_multi"], n), d["ws_buf"])
        be.gan_reduce_grad_multi(kinds, As, Bs, scale,
                                 outs=[inner(gm[i], t["rows"] * t["width"]) for i, t in enumerate(terms)])
        o["sum_ops"] = be.gan_reduce_multi(kinds, As, Bs, scale).cpu()
        for k in d:
            o[k] = d[k].cpu()
        o["g_single"], o["g_multi"] = [x.cpu() for x in gs], [x.cpu() for x in gm]
    m["a_buf"] = [x.cpu() for x in a_buf]
    m["b_buf"] = [None if x is None else x.cpu() for x in b_buf]


def _guard_hit(buf, lo, n):
    raw = _bits(buf)
    want = _bits(_pattern(buf.numel(), buf.dtype))
    bad = raw != want
    bad[lo:lo + n] = False
    return int(bad.nonzero()[0]) if bool(bad.any()) else None


def verify(c, m, ref):
    """Raises AssertionError naming the case and the first failed check of FAILURES; returns the worst
    |got - S| / bar over the sums."""
    nm, terms = c["name"], c["terms"]
    n = len(terms)
    for r, o in enumerate(m["outs"]):
        bufs = [("sum_single", o["sum_single"], GUARD_N, n), ("sum_acc", o["sum_acc"], GUARD_N, n),
                ("sum_multi", o["sum_multi"], GUARD_N, n), ("ws_buf", o["ws_buf"][m["ws_floats"]:], 0, 0)]
        for key in ("g_single", "g_multi"):
            bufs += [(f"{key}[{i}]", o[key][i], GUARD_N, t["rows"] * t["width"]) for i, t in enumerate(terms)]
        for key, buf, lo, k in bufs:
            hit = _guard_hit(buf, lo, k)
            assert hit is None, f"{nm}: guard: run {r} wrote {key}[{hit}]"
    for key in ("a", "b"):
        for i in range(n):
            now, was = m[key + "_buf"][i], m[key + "_orig"][i]
            assert now is None or torch.equal(_bits(now), _bits(was)), f"{nm}: operand: {key}_buf[{i}] changed"
    o = m["outs"][0]
    for key in ("g_single", "g_multi"):
        for i, t in enumerate(terms):
            got = o[key][i][GUARD_N:GUARD_N + t["rows"] * t["width"]].view(t["rows"], t["width"])
            bad = _bits(got) != _bits(ref["grad"][i])
            assert not bool(bad.any()), f"{nm}: gradient: {key}[{i}] (kind {t['kind']}): {int(bad.sum())} of " \
                                        f"{bad.numel()} elements differ, first at " \
                                        f"{tuple(int(j) for j in bad.nonzero()[0])}"
    worst = 0.0
    for key in ("sum_single", "sum_multi"):
        got = o[key][GUARD_N:GUARD_N + n].double()
        for i, t in enumerate(terms):
            f = t["scale"] if key == "sum_multi" else 1.0
            err, bar = abs(float(got[i]) - f * ref["S"][i]), abs(f) * ref["bar"][i]
            print(f"{nm}: {key}[{i}]: error {err:.3e}, bar {bar:.3e}")
            worst = max(worst, err / bar)
            assert err <= bar, f"{nm}: sum bar: {key}[{i}] = {float(got[i])!r}, S = {f * ref['S'][i]!r}: " \
                               f"error {err:.3e} > bar {bar:.3e}"
    s = o["sum_single"][GUARD_N:GUARD_N + n]
    want = torch.full((n,), ACC0, dtype=torch.float32) + s
    same = torch.equal(_bits(o["sum_acc"][GUARD_N:GUARD_N + n]), _bits(want))
    assert same, f"{nm}: accumulate: into {ACC0} gives {o['sum_acc'][GUARD_N:GUARD_N + n].tolist()}, " \
                 f"fp32 {ACC0} + sum is {want.tolist()}"
    same = torch.equal(_bits(o["sum_ops"]), _bits(o["sum_multi"][GUARD_N:GUARD_N + n]))
    assert same, f"{nm}: multi: ops.gan_reduce_multi differs from the call with the caller's buffers"
    o2 = m["outs"][1]
    for key in ("sum_single", "sum_acc", "sum_multi", "sum_ops"):
        assert torch.equal(_bits(o[key]), _bits(o2[key])), f"{nm}: determinism: {key} of the second run differs"
    for key in ("g_single", "g_multi"):
        for i in range(n):
            assert torch.equal(_bits(o[key][i]), _bits(o2[key][i])), f"{nm}: determinism: {key}[{i}] differs"
    return worst


# ---- the CPU stand-in for the kernels, and its deliberate faults

# drop_unit / double_unit: the last unit (8-element vector, or element) of term 0 is left out of / counted twice
# in its sum.  neighbour_kind: term 0 is read with the kind of the next term (of kind + 1 where it is alone).
# tie_sign: the gradient at a tie of kind 0 is +scale.  pad_write: the gradient kernel writes the first padding
# element of a strided a.  no_scale: the gradients and the multi sums miss the term's scale.  guard_*: one element
# past a gradient, before the output vector, past the queried workspace.  no_accumulate: vo_gan_reduce overwrites.
# second_run_differs: one ulp on one sum of the second run.
MUTATIONS = {  # name -> the failure verify must name
    "drop_unit": "sum bar", "double_unit": "sum bar", "neighbour_kind": "gradient", "tie_sign": "gradient",
    "pad_write": "operand", "no_scale": "gradient", "guard_grad": "guard", "guard_out": "guard",
    "guard_ws": "guard", "no_accumulate": "accumulate", "second_run_differs": "determinism"}


def applies(c, mutate):
    """Whether the fault changes anything the checker can see on this case."""
    t = c["terms"]
    return {"drop_unit": not c["grad_cap"], "double_unit": not c["grad_cap"],
            "tie_sign": any(x["special"] and x["kind"] == 0 and x["scale"] != 0 for x in t),
            "pad_write": any(x["lda"] > x["width"] and x["rows"] > 1 for x in t),
            "no_scale": any(x["scale"] != 1.0 for x in t)}.get(mutate, True)


class Standin:
    """The four entry points in plain fp32 torch on the CPU, on the operands as laid out in memory."""

    def __init__(self, c, m, mutate=None):
        self.c, self.m, self.mutate, self.calls = c, m, mutate, 0

    def _kind(self, i):
        if self.mutate == "neighbour_kind" and i == 0:
            k = self.c["terms"][1]["kind"] if len(self.c["terms"]) > 1 else (self.c["terms"][0]["kind"] + 1) % 3
            return k if k != self.c["terms"][0]["kind"] else (k + 1) % 3
        return self.c["terms"][i]["kind"]

    def _index(self, a):
        return next(i for i, t in enumerate(self.c["terms"])
                    if a.data_ptr() == view(self.m["a_buf"][i], t).data_ptr())

    def _sum(self, i, a, b):
        t, k = self.c["terms"][i], self._kind(i)
        y = b.float() if b is not None else (a.float() * 0 if k == 0 else None)
        v = values(k, a.float(), y).reshape(-1)
        s = v.sum()
        if i == 0 and self.mutate in ("drop_unit", "double_unit"):
            tail = v[-chain(self.c, t)[0]:].sum()
            s = s - tail if self.mutate == "drop_unit" else s + tail
        return s

    def gan_reduce(self, kind, a, b=None, out=None):
        s = self._sum(self._index(a), a, b)
        self.calls += 1
        if self.mutate == "second_run_differs" and self.calls == 2 * len(self.c["terms"]) + 1:
            s = torch.nextafter(s, torch.tensor(float("inf")))
        if self.mutate == "no_accumulate":
            out.copy_(s)
        else:
            out += s
        return out

    def _grad(self, i, a, b, s, out):
        t, k = self.c["terms"][i], self._kind(i)
        s = s.float() if self.mutate != "no_scale" else torch.ones((), dtype=torch.float32)
        y = b.float() if b is not None else (a.float() * 0 if k == 0 else None)
        g = grad32(k, a.float(), y, s)
        if self.mutate == "tie_sign" and k == 0:
            g = torch.where(a.float() == y, s, g)
        out.view(t["rows"], t["width"]).copy_(g.to(out.dtype))
        if self.mutate == "pad_write" and t["lda"] > t["width"] and t["rows"] > 1:
            self.m["a_buf"][i][t["off"] + t["width"]] = 0.0
        if self.mutate == "guard_grad" and i == 0:
            _bits(out.as_strided((1,), (1,), out.storage_offset() + out.numel()))[0] += 1
        return out

    def gan_reduce_grad(self, kind, a, b, scale, out=None):
        return self._grad(self._index(a), a, b, scale, out)

    def gan_reduce_grad_multi(self, kinds, As, Bs, scale, outs=None):
        return [self._grad(i, As[i], Bs[i], scale[i], outs[i]) for i in range(len(kinds))]

    def gan_reduce_multi_into(self, kinds, As, Bs, scale, out, ws):
        for i in range(len(kinds)):
            s = self._sum(i, As[i], Bs[i])
            out[i] = s if self.mutate == "no_scale" else s * scale[i]
        ws[:self.m["ws_floats"]] = 0.0
        if self.mutate == "guard_out":
            _bits(out.as_strided((1,), (1,), out.storage_offset() - 1))[0] += 1
        if self.mutate == "guard_ws":
            ws.view(torch.int32)[self.m["ws_floats"]] += 1

    def gan_reduce_multi(self, kinds, As, Bs, scale=None):
        out = torch.empty(len(kinds), dtype=torch.float32)
        mutate, self.mutate = self.mutate, (self.mutate if self.mutate in ("drop_unit", "double_unit", "no_scale",
                                                                            "neighbour_kind") else None)
        self.gan_reduce_multi_into(kinds, As, Bs, scale, out, torch.empty(self.m["ws_floats"] + 1))
        self.mutate = mutate
        return out
