"""Checker of one vo_conv1d call against float64, with a derived element-wise bar and guard bands.

A case is a dict (see ``case``).  ``make`` draws its operands on the CPU and lays them out with guards,
``reference`` computes the float64 result and the bar, ``run`` hands the views to a conv function (the
GPU op, or in the CPU self-test ``torch_conv``) and ``verify`` checks values and guards.

Reference: for bf16 compute every operand is bf16-exact (rounded before the reference sees it; an fp32
input to a bf16-compute conv is bf16-exact too), the prologue activation is applied in fp32 and rounded
to bf16 as the kernel stages it, the conv is F.conv1d in float64, the epilogue
(act(acc + bias) + res1) * scale + res2 in float64.

Element bar: |got - ref| <= 2 (R + 8) 2^-24 A, R = (Ci / groups) K, A the same expression on absolute
values (conv(|x|, |w|) + |b| + |res1|) |scale| + |res2| -- the any-order fp32 dot-product bound (the
+ 8 covers the epilogue's roundings, the factor 2 accumulator adds that truncate).  relu / leaky-ReLU
(slope in [0, 1]) and tanh are 1-Lipschitz, so the bound on acc + bias carries through them; tanh adds
5 ulp of its fp32 result (the OpenCL full-profile bound of tanh the device math library follows), the one
term for arithmetic the dot-product bound does not model.  bf16 output adds 2^-8 |ref| (RNE half ulp).
Whole-tensor bar (fp32 output): rel-L2 < 1e-5, the project's fp32 module tolerance -- the element bound
is loose for deep reductions, this one is not.
"""

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
REL_L2_F32 = 1e-5
X_GUARD = 1e4                      # finite: ragged kernels multiply clamped loads by zeroed weights
Y_GUARD = {torch.float32: 0x5A5AA5A5, torch.bfloat16: 0x5A5B}  # a fixed bit pattern (finite in both formats)
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def case(B, T, Ci, Co, K, *, dil=1, pad=None, stride=1, groups=1, T_out=None, cdt="bf16", xdt=None, ydt="f32",
         bias=True, res1=False, res2=False, scale=1.0, post=ACT_NONE, post_slope=0.0, pre=ACT_NONE, pre_slope=0.1,
         ldx_extra=0, x_rows=0, ldy_extra=0, y_rows=1, tile=None, wave=None, seed=None, name=None):
    """pad None = dil (K - 1) / 2; ldx_extra: sentinel channels [Ci, ldx); x_rows: sentinel rows before and
    after each utterance of x (a T-sliced x); ldy_extra: guard channels [Co, ldy) (row-strided out view, no
    residuals); y_rows: guard rows after each utterance's T_out rows when the view is row-strided (no
    residuals), and guard utterances around the batch always; tile: the expected launch record fields
    (BCO, BT, S, SEG, nice, splits) and wave its (NI, WCO)."""
    xdt = xdt or cdt
    c = dict(B=B, T=T, Ci=Ci, Co=Co, K=K, dil=dil, pad=dil * (K - 1) // 2 if pad is None else pad, stride=stride,
             groups=groups, cdt=cdt, xdt=xdt, ydt=ydt, bias=bias, res1=res1, res2=res2, scale=scale, post=post,
             post_slope=post_slope, pre=pre, pre_slope=pre_slope, ldx_extra=ldx_extra, x_rows=x_rows,
             ldy_extra=ldy_extra, y_rows=y_rows, tile=tile, wave=wave)
    nat = (T + 2 * c["pad"] - dil * (K - 1) - 1) // stride + 1
    c["T_out"] = nat if T_out is None else T_out
    c["T_out_arg"] = T_out
    c["seed"] = seed if seed is not None else (B * 1000003 + T * 1009 + Ci * 31 + Co * 7 + K) % (2 ** 31)
    c["name"] = name or (f"{xdt}-{cdt}-{ydt}_B{B}_T{T}_Ci{Ci}_Co{Co}_K{K}" + (f"_d{dil}" if dil > 1 else "") +
                         (f"_s{stride}" if stride > 1 else "") + (f"_g{groups}" if groups > 1 else ""))
    if (res1 or res2) and ldy_extra:
        raise ValueError("residuals need a contiguous output")
    return c


def record(c):
    """The launch record vo_conv1d must report for the case (ops.LAUNCH_FIELDS order)."""
    bco, bt, s, seg, nice, splits = c["tile"]
    ni, wco = c["wave"]
    size = {"bf16": 2, "f32": 4}
    return dict(BCO=bco, BT=bt, S=s, SEG=seg, nice=nice, splits=splits, sizeof_in=size[c["xdt"]],
                sizeof_compute=size[c["cdt"]], sizeof_out=size[c["ydt"]], ROLE=0,
                compute_dtype={"f32": 0, "bf16": 1}[c["cdt"]], NI=ni, WCO=wco)


def instantiation(c):
    """(NI, WCO, BT, S, SEG, nice, sizeof TIN, TC, TOUT): one conv1d_kernel instantiation (BCO = 16 NI WCO;
    NI and WCO tell apart tiles of equal BCO x BT, e.g. the Co = 80 and the default bf16 64 x 128 tiles)."""
    r = record(c)
    return (r["NI"], r["WCO"], r["BT"], r["S"], r["SEG"], r["nice"], r["sizeof_in"], r["sizeof_compute"],
            r["sizeof_out"])


def x_view(c, x_buf):
    return x_buf[:, c["x_rows"]:c["x_rows"] + c["T"], :]


def y_view(c, y_buf):
    return y_buf[1:c["B"] + 1, :c["T_out"], :c["Co"]]


def _exact(t, c):
    return t.bfloat16().float() if c["cdt"] == "bf16" else t


def make(c):
    """CPU operands of the case.  x / out / res are views into guarded buffers."""
    g = torch.Generator().manual_seed(c["seed"])
    B, T, Ci, Co, K, G = c["B"], c["T"], c["Ci"], c["Co"], c["K"], c["groups"]
    cig = Ci // G
    xdt, ydt = DT[c["xdt"]], DT[c["ydt"]]
    x = _exact(torch.randn(B, T, Ci, generator=g), c)
    w = _exact(torch.randn(Co, cig, K, generator=g) / (cig * K) ** 0.5, c)
    b = torch.randn(Co, generator=g) * 0.1 if c["bias"] else None
    m = dict(w=w, bias=b)
    # x: (B, x_rows + T + x_rows, Ci + ldx_extra) filled with the sentinel, the view in the middle
    xr, ldx = c["x_rows"], Ci + c["ldx_extra"]
    xbuf = torch.full((B, T + 2 * xr, ldx), X_GUARD, dtype=xdt)
    xbuf[:, xr:xr + T, :Ci] = x.to(xdt)
    m["x_buf"], m["x"] = xbuf, x_view(c, xbuf)
    m["x_val"] = x
    # packed weights [K][Co][Ci], block-diagonal for groups
    wp = torch.zeros(K, Co, Ci)
    cog = Co // G
    for gi in range(G):
        wp[:, gi * cog:(gi + 1) * cog, gi * cig:(gi + 1) * cig] = w[gi * cog:(gi + 1) * cog].permute(2, 0, 1)
    m["w_packed"] = wp.to(DT[c["cdt"]]).contiguous()
    # out: guard utterances around the batch; row-strided (guard rows / channels) where there are no residuals
    To = c["T_out"]
    strided = not (c["res1"] or c["res2"])
    yr = c["y_rows"] if strided else 0
    ldy = Co + (c["ldy_extra"] if strided else 0)
    ybuf = torch.empty((B + 2, To + yr, ldy), dtype=ydt)
    ybuf.view(_INT[ydt]).fill_(Y_GUARD[ydt])
    m["y_buf"], m["y"] = ybuf, y_view(c, ybuf)
    m["y_mask"] = torch.zeros(ybuf.shape, dtype=torch.bool)
    m["y_mask"][1:B + 1, :To, :Co] = True
    for r in ("res1", "res2"):
        m[r] = (torch.randn(B, To, Co, generator=g)).to(ydt) if c[r] else None
    return m


def _act64(v, kind, slope):
    if kind == ACT_RELU:
        return v.clamp_min(0)
    if kind == ACT_LRELU:
        return torch.maximum(v, v * float(np.float32(slope)))
    if kind == ACT_TANH:
        return torch.tanh(v)
    return v


def staged_input(c, x):
    """x as the kernel stages it: prologue activation in fp32, rounded to the compute type."""
    if c["pre"] == ACT_NONE:
        return x.float()
    s = torch.tensor(0.0 if c["pre"] == ACT_RELU else c["pre_slope"], dtype=torch.float32)
    v = torch.maximum(x.float(), x.float() * s)
    return _exact(v, c)


def _conv64(c, x, w):
    """float64 conv of channels-last x (B, T, Ci) with w (Co, Ci / groups, K): T_out rows, rows outside
    [0, T) read as zero (a T_out past the natural length reads zeros on the right)."""
    S, dil, K, pad, To = c["stride"], c["dil"], c["K"], c["pad"], c["T_out"]
    need = (To - 1) * S + dil * (K - 1) + 1
    xt = F.pad(x.double().transpose(1, 2), (pad, max(need - pad - x.shape[1], 0)))
    y = F.conv1d(xt, w.double(), None, stride=S, dilation=dil, groups=c["groups"])
    return y[:, :, :To].transpose(1, 2)


def reference(c, m):
    """(ref, bar) in float64; bar is the element-wise bound of the module docstring."""
    xs = staged_input(c, m["x_val"])
    acc = _conv64(c, xs, m["w"])
    A = _conv64(c, xs.abs(), m["w"].abs())
    if m["bias"] is not None:
        acc = acc + m["bias"].double()
        A = A + m["bias"].double().abs()
    v = _act64(acc, c["post"], c["post_slope"])
    extra = 5 * 2.0 ** -23 * v.abs() if c["post"] == ACT_TANH else 0.0
    if m["res1"] is not None:
        v = v + m["res1"].double()
        A = A + m["res1"].double().abs()
    sc = float(np.float32(c["scale"]))
    v, A, extra = v * sc, A * abs(sc), extra * abs(sc)
    if m["res2"] is not None:
        v = v + m["res2"].double()
        A = A + m["res2"].double().abs()
    R = (c["Ci"] // c["groups"]) * c["K"]
    bar = 2 * (R + 8) * 2.0 ** -24 * A + extra
    if c["ydt"] == "bf16":
        bar = bar + 2.0 ** -8 * v.abs()
    return v, bar


def verify(c, m, ref, bar):
    """Values inside the view against (ref, bar), everything outside bit-identical to the guard pattern, the
    input buffer unchanged.  Returns (worst error / bar, rel-L2); raises AssertionError."""
    ydt = DT[c["ydt"]]
    raw = m["y_buf"].view(_INT[ydt])
    touched = (raw != Y_GUARD[ydt]) & ~m["y_mask"]
    assert not bool(touched.any()), f"{c['name']}: {int(touched.sum())} guard elements written, first at " \
                                    f"{tuple(int(i) for i in touched.nonzero()[0])} of {tuple(raw.shape)}"
    got = m["y"].double()
    assert bool(torch.isfinite(got).all()), f"{c['name']}: non-finite output"
    err = (got - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    print(f"{c['name']}: worst error/bar {ratio:.3e}, rel-L2 {rel:.3e}")
    over = err > bar
    assert not bool(over.any()), f"{c['name']}: {int(over.sum())} of {over.numel()} elements over the bar " \
                                 f"(worst ratio {ratio:.3g}), first at {tuple(int(i) for i in over.nonzero()[0])}"
    if c["ydt"] == "f32":
        assert rel < REL_L2_F32, f"{c['name']}: rel-L2 {rel:.3e} >= {REL_L2_F32}"
    return ratio, rel


def conv_kwargs(c):
    """Keyword arguments of ops.conv1d for the case (without tensors)."""
    kw = dict(Co=c["Co"], K=c["K"], dil=c["dil"], pad=c["pad"], pre_act=c["pre"], pre_slope=c["pre_slope"],
              post_act=c["post"], post_slope=c["post_slope"], out_scale=c["scale"], compute_dtype=DT[c["cdt"]],
              stride=c["stride"], groups=c["groups"])
    if c["T_out_arg"] is not None:
        kw["T_out"] = c["T_out_arg"]
    return kw


def torch_conv(c, m, mutate=None):
    """The CPU stand-in for the kernel in the self-test: F.conv1d in fp32 on the operands as laid out in
    memory (the x view with its ldx channels, the packed weights), written into the out view.  ``mutate``
    names a deliberate fault."""
    Ci, K, To = c["Ci"], c["K"], c["T_out"]
    xv = m["x"]
    if mutate == "shift_row":  # the window starts one row early: reads the row before each utterance
        xv = m["x_buf"][:, c["x_rows"] - 1:c["x_rows"] - 1 + c["T"], :]
    nch = Ci + 1 if mutate == "leak_channel" else Ci
    xs = staged_input(c, xv[:, :, :nch].float())
    w = m["w_packed"].float().permute(1, 2, 0)  # dense (Co, Ci, K), zeros outside the groups
    if mutate == "leak_channel":  # a weight column that should have been zeroed multiplies channel Ci
        w = torch.cat([w, w[:, :1, :]], dim=1)
    if mutate == "drop_tap":
        w = w.clone()
        w[:, :, K - 1] = 0
    if mutate == "drop_channel":
        w = w.clone()
        w[:, Ci - 1, :] = 0
    S, dil, pad = c["stride"], c["dil"], c["pad"]
    need = (To - 1) * S + dil * (K - 1) + 1
    xt = F.pad(xs.transpose(1, 2), (pad, max(need - pad - xs.shape[1], 0)))
    v = F.conv1d(xt, w, None, stride=S, dilation=dil)[:, :, :To].transpose(1, 2)
    if m["bias"] is not None:
        v = v + m["bias"]
    v = _act64(v, c["post"], c["post_slope"]).float()
    if m["res1"] is not None:
        v = v + m["res1"].float()
    v = v * np.float32(c["scale"])
    if m["res2"] is not None:
        v = v + m["res2"].float()
    if mutate == "zero_group":  # one 4-channel group of the last output row
        v = v.clone()
        v[-1, -1, c["Co"] - 4:] = 0
    m["y"].copy_(v.to(m["y"].dtype))
    if mutate == "guard":
        flat = m["y_buf"].view(_INT[DT[c["ydt"]]])
        flat[-1, 0, 0] += 1
