"""Torch-tensor front end of the C ABI: shape checks, output allocation, stream plumbing.

Every function here launches a hand-written HIP kernel from ``lib/libvonoma.so`` on
the current torch stream of the tensors' device.  Tensors must be CUDA (ROCm)
tensors; there is no CPU path -- a CPU tensor raises.
"""

import ctypes

import numpy as np

import torch

from . import _lib, profiling
from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, HEAD_DURATION, HEAD_ENERGY,  # noqa: F401
                   PACK_CONV, PACK_CONVT, VO_BF16, VO_F32, VO_F32X3)

_DT = {torch.float32: VO_F32, torch.bfloat16: VO_BF16}


class _F32X3:
    """``compute_dtype`` of a contraction over fp32 tensors computed as split-bf16 (VO_F32X3 in
    include/vonoma.h): each fp32 operand as hi + lo bf16, three bf16 MFMAs per product, <= 3 * 2^-18
    relative error per product.  Tensors, packed weights and results stay fp32 (storage_dtype)."""

    def __repr__(self):
        return "ops.F32X3"


F32X3 = _F32X3()


def storage_dtype(cdt):
    """The torch dtype of the tensors and packed weights of compute dtype ``cdt``."""
    return torch.float32 if cdt is F32X3 else cdt


def vo_dtype(t):
    try:
        return _DT[t if isinstance(t, torch.dtype) else t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t}") from None


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    if not t.is_cuda:
        raise RuntimeError("visual_onoma_to_wave_amd ops run on the GPU only (got a CPU tensor); "
                           "there is no CPU fallback")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _contig(t, name):
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _check_lens(lens, lens_scale, B, ref, name):
    """Validate the per-utterance lengths of a ragged call: a contiguous int32 (B,) tensor on ``ref``'s device
    (never read on the host) and an integer lens_scale >= 1."""
    if not isinstance(lens, torch.Tensor):
        raise TypeError(f"{name}: lens must be a device tensor (a host sequence goes through Generator.run)")
    if lens.dtype != torch.int32:
        raise TypeError(f"{name}: lens must be int32, got {lens.dtype}")
    if lens.dim() != 1 or lens.shape[0] != B:
        raise ValueError(f"{name}: lens must have shape ({B},), got {tuple(lens.shape)}")
    if lens.device != ref.device:
        raise ValueError(f"{name}: lens is on {lens.device}, the activations on {ref.device}")
    _contig(lens, "lens")
    if int(lens_scale) != lens_scale or lens_scale < 1:
        raise ValueError(f"{name}: lens_scale must be an integer >= 1, got {lens_scale}")
    return int(lens_scale)


# ----------------------------------------------------------------------------- conv1d

def _conv1d_desc(x, w_packed, bias, *, Co, K, dil=1, pad=0, T_out=None, out=None, out_dtype=None,
                 pre_act=ACT_NONE, pre_slope=0.0, post_act=ACT_NONE, post_slope=0.0, res1=None,
                 res2=None, out_scale=1.0, compute_dtype=torch.bfloat16, transposed=None, variant=0,
                 stride=1, groups=1, ymask=None, ymask_slope=0.0, lens=None, lens_scale=1):
    """The vo_conv1d_desc of a ``conv1d`` call (its keyword arguments and defaults), shape checks and output
    allocation included.  Returns (d, x, out, ws_bytes): ws_bytes > 0 = the split-reduction scratch the call wants
    (d.workspace is left for the caller to set)."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, T_in, ldx = x.shape
    if x.stride(2) != 1 or x.stride(1) != ldx:
        raise ValueError("conv1d: x must be row-contiguous (B, T, C)")
    Ci = w_packed.shape[2]
    if w_packed.shape[0] != K or w_packed.shape[1] != Co:
        raise ValueError(f"conv1d: packed weight {tuple(w_packed.shape)} != [{K}][{Co}][Ci]")
    if w_packed.dtype != storage_dtype(compute_dtype):
        raise ValueError("conv1d: packed weight dtype must equal the compute dtype")
    if compute_dtype is F32X3 and (x.dtype != torch.float32 or stride > 1 or groups > 1 or transposed is not None):
        raise ValueError("conv1d: F32X3 compute needs fp32 input, stride 1, no groups, not transposed")
    out_dtype = out_dtype or x.dtype
    if transposed is not None:
        s, p, cout = transposed["stride"], transposed["pad"], transposed["cout"]
        T_rows = T_in + 1
        up_tout = transposed.get("tout", T_in * s + s - 2 * p)
        shape = (B, up_tout, cout)
        ldy = cout
    else:
        T_rows = T_out if T_out is not None else (T_in + 2 * pad - dil * (K - 1) - 1) // stride + 1
        shape = (B, T_rows, Co)
        ldy = Co
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    if out.dim() == 2:
        out = out.unsqueeze(0)
    if transposed is None and not out.is_contiguous():
        # row-strided output view (phase-interleaved rows of a strided conv's input gradient):
        # rows ldy elements apart, channels contiguous; no residuals on such views
        if out.stride(2) != 1 or out.shape[2] != Co or res1 is not None or res2 is not None:
            raise ValueError("conv1d: a non-contiguous out must be a row-strided (B, T, Co) view")
        ldy = out.stride(1)
    else:
        _contig(out, "out")
    if res1 is not None and (res1.shape != out.shape or res1.dtype != out.dtype):
        raise ValueError("conv1d: res1 must match the output")
    if res2 is not None and (res2.shape != out.shape or res2.dtype != out.dtype):
        raise ValueError("conv1d: res2 must match the output")
    d = _lib.Conv1dDesc()
    d.x = x.data_ptr(); d.x_dtype = vo_dtype(x); d.x_bstride = x.stride(0); d.ldx = ldx
    d.w = w_packed.data_ptr(); d.bias = bias.data_ptr() if bias is not None else None
    d.y = out.data_ptr(); d.y_dtype = vo_dtype(out); d.y_bstride = out.stride(0); d.ldy = ldy
    d.res1 = res1.data_ptr() if res1 is not None else None
    d.res2 = res2.data_ptr() if res2 is not None else None
    d.B, d.T_in, d.T_out, d.Ci, d.Co = B, T_in, T_rows, Ci, Co
    d.K, d.dil, d.pad = K, dil, pad
    d.pre_act, d.pre_slope, d.post_act, d.post_slope = pre_act, pre_slope, post_act, post_slope
    d.out_scale = out_scale
    d.compute_dtype = VO_F32X3 if compute_dtype is F32X3 else vo_dtype(compute_dtype)
    if transposed is not None:
        d.transposed, d.up_stride, d.up_pad, d.up_cout, d.up_tout = 1, s, p, cout, up_tout
    d.variant = variant if (x.dtype == out.dtype == compute_dtype == torch.bfloat16) else 0
    d.stride, d.groups = stride, groups
    if ymask is not None:
        if ymask.dim() == 2:
            ymask = ymask.unsqueeze(0)
        if ymask.shape != out.shape or ymask.stride() != out.stride() or ymask.dtype != out.dtype:
            raise ValueError("conv1d: ymask must match the output (shape, strides, dtype)")
        d.ymask, d.ymask_slope = ymask.data_ptr(), float(ymask_slope)
    if lens is not None:
        d.lens_scale = _check_lens(lens, lens_scale, B, x, "conv1d")
        d.lens = lens.data_ptr()
    plain = (transposed is None and stride <= 1 and groups <= 1 and lens is None)
    deep_bf16 = (compute_dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and bias is None and res1 is None and
                 res2 is None and ymask is None and pre_act == ACT_NONE and post_act == ACT_NONE and out_scale == 1.0 and
                 Co <= 256 and Ci * K >= 2048 and B * T_rows >= 8192)
    ws_bytes = 0
    if plain and ((storage_dtype(compute_dtype) == torch.float32 and T_rows <= 16) or deep_bf16):
        # split-reduction scratch: the short fp32 convs, the deep bf16 convs into <= 256 channels
        ws_bytes = int(_lib.lib().vo_conv1d_workspace_size(ctypes.byref(d)))
    return d, x, out, ws_bytes


def conv1d(x, w_packed, bias, *, tag=None, **kw):
    """Channels-last conv: x (B, T_in, Ci) -> y (B, T_out, Co).  Keyword arguments (defaults in _conv1d_desc):
    Co, K, dil=1, pad=0, T_out, out, out_dtype, pre_act, pre_slope, post_act, post_slope, res1, res2, out_scale=1.0,
    compute_dtype=torch.bfloat16, transposed, variant=0, stride=1, groups=1, ymask, ymask_slope, lens, lens_scale=1;
    ``tag`` names the call for the profiling timer.

    ``w_packed``: [K][Co][Ci] in ``compute_dtype`` (see pack_conv_weight).
    ``transposed``: None or dict(stride=s, pad=p, cout=C_out) for the polyphase
    ConvTranspose1d; then Co = s*C_out, K = 2, pad = 1 and y is (B, s*T_in, C_out).
    ``stride`` / ``groups``: strided and grouped convs (HiFi-GAN discriminators); grouped
    weights are packed dense with zeros outside the diagonal blocks (pack_conv_weight groups=).
    ``ymask`` (the output's shape and strides, bf16): each output stored as
    round(round(v) * (ymask > 0 ? 1 : ymask_slope)) -- an input gradient put through the leaky-ReLU
    backward of the layer whose output ymask is (bit for bit vo_lrelu_mask on the stored output).
    ``lens`` (int32 (B,) on the device) / ``lens_scale``: ragged batch -- utterance b is the tensor of its first
    clamp(lens[b] * lens_scale, 0, T_in) rows: rows past it read as zero (x, res1, res2) and are not written
    (include/vonoma.h, "per-utterance lengths"; same-length convs and the polyphase form only).  The profiling
    timer's FLOPs and bytes of a ragged call are still those of the padded shape: a true count would need the
    lengths on the host.
    """
    d, x, out, ws_bytes = _conv1d_desc(x, w_packed, bias, **kw)
    if ws_bytes > 0:  # stream-ordered: freed after enqueue
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
    timer = profiling.active()
    ev = timer.start() if (tag is not None and timer is not None and timer.watching(tag)) else None
    _lib.check(_lib.lib().vo_conv1d(ctypes.byref(d), _stream(x)), "vo_conv1d")
    if ev is not None:
        res1, res2 = kw.get("res1"), kw.get("res2")
        flops = 2.0 * d.B * d.T_out * d.Co * d.Ci * d.K / kw.get("groups", 1)
        nbytes = (d.B * d.T_in * d.Ci * x.element_size() + out.numel() * out.element_size() +
                  (res1.numel() * res1.element_size() if res1 is not None else 0) +
                  (res2.numel() * res2.element_size() if res2 is not None else 0) +
                  w_packed.numel() * w_packed.element_size())
        timer.stop(tag, ev, flops, nbytes, kernel=f"conv1d_kernel<..., ROLE={d.variant}>")
    return out


LAUNCH_FIELDS = ("BCO", "BT", "S", "SEG", "nice", "splits", "sizeof_in", "sizeof_compute", "sizeof_out", "ROLE",
                 "compute_dtype", "NI", "WCO")


def conv1d_plan(x, w_packed, bias, *, tag=None, **kw):
    """The launch record ``conv1d`` with the same arguments would leave (a dict over LAUNCH_FIELDS), without
    launching anything: the same descriptor, workspace decision included, through vo_conv1d_plan -- the dispatcher's
    host side alone.  All zeros for a call the streaming upsampler takes; raises where ``conv1d`` would."""
    d, x, _, ws_bytes = _conv1d_desc(x, w_packed, bias, **kw)
    if ws_bytes > 0:  # never dereferenced: the plan only asks whether a workspace of that size is set
        d.workspace, d.workspace_bytes = d.y, ws_bytes
    rec = (ctypes.c_int32 * len(LAUNCH_FIELDS))()
    _lib.check(_lib.lib().vo_conv1d_plan(ctypes.byref(d), rec, len(LAUNCH_FIELDS)), "vo_conv1d_plan")
    return dict(zip(LAUNCH_FIELDS, (int(v) for v in rec)))


def conv1d_plane_takes(x, w_packed, bias, *, tag=None, **kw):
    """Whether ``conv1d`` with the same arguments runs on the plane conv (vo_conv1d_plane_takes in
    include/vonoma.h: MRF stage 0 in the wave-owned output-plane form); host only, launches nothing."""
    d, x, _, ws_bytes = _conv1d_desc(x, w_packed, bias, **kw)
    if ws_bytes > 0:  # never dereferenced, as in conv1d_plan
        d.workspace, d.workspace_bytes = d.y, ws_bytes
    return bool(_lib.lib().vo_conv1d_plane_takes(ctypes.byref(d)))


def conv1d_last_launch():
    """The tile the calling thread's last ``conv1d`` launched, as a dict over LAUNCH_FIELDS
    (vo_conv1d_last_launch in include/vonoma.h); all zeros when the call was rejected or went to the
    streaming upsampler."""
    rec = (ctypes.c_int32 * len(LAUNCH_FIELDS))()
    n = _lib.lib().vo_conv1d_last_launch(rec, len(LAUNCH_FIELDS))
    if n != len(LAUNCH_FIELDS):
        raise RuntimeError(f"vo_conv1d_last_launch returned {n} fields, expected {len(LAUNCH_FIELDS)}")
    return dict(zip(LAUNCH_FIELDS, (int(v) for v in rec)))


def pack_dgrad_weight(w, dtype):
    """(Co, Ci, K) -> [K][Ci][Co] taps reversed: dX = conv1d(dY, this, Co=Ci, pad=(K-1)*dil - pad)."""
    w = w.detach().float().contiguous()
    Co, Ci, K = w.shape
    out = torch.empty((K, Ci, Co), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().vo_pack_weight(_ptr(w), None, None, 2, Co, Ci, K, 1, _ptr(out), vo_dtype(dtype),
                                         _stream(w)), "vo_pack_weight")
    return out


def pack_conv_weight(w, dtype, g=None, row_scale=None, transposed_stride=None):
    """(Co, Ci, K) Conv1d weight (or (Ci, Co, 2s) ConvTranspose1d weight) -> packed.

    g: weight-norm gains (one per dim-0 slice), row_scale: per-output-channel multiplier.
    Returns [K][Co][Ci] (conv) or [2][s*Co][Ci] (transposed) in ``dtype``.
    """
    w = w.detach().float().contiguous()
    if transposed_stride is None:
        Co, Ci, K = w.shape
        out = torch.empty((K, Co, Ci), dtype=dtype, device=w.device)
        mode, stride = PACK_CONV, 1
    else:
        Ci, Co, K = w.shape
        s = transposed_stride
        out = torch.empty((2, s * Co, Ci), dtype=dtype, device=w.device)
        mode, stride = PACK_CONVT, s
    g = None if g is None else g.detach().float().reshape(-1).contiguous()
    rs = None if row_scale is None else row_scale.detach().float().reshape(-1).contiguous()
    _lib.check(_lib.lib().vo_pack_weight(_ptr(w), _ptr(g), _ptr(rs), mode, Co, Ci, K, stride,
                                         _ptr(out), vo_dtype(dtype), _stream(w)), "vo_pack_weight")
    return out


# ----------------------------------------------------------------------------- layer norm

def _ln_fwd(name, x, res, y_dtype, with_bf16, out=None):
    """What the forward wrappers share: x and res contiguous and of one shape; y (``out`` if given) and, with_bf16,
    its bf16 copy.  Returns (y, y16 or None)."""
    _contig(x, "x")
    if res is not None:
        _contig(res, "res")
        if res.shape != x.shape:
            raise ValueError(f"{name}: res shape mismatch")
    y = out if out is not None else torch.empty(x.shape, dtype=y_dtype, device=x.device)
    return y, torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if with_bf16 else None


def _ln_bwd(name, x, gy, res, gy2=None, gres_dtype=None):
    """What the backward wrappers share, before any launch: x, gy, res and gy2 contiguous, gy and res of x's shape,
    gy2 bf16 of x's shape (the kernels read it as bf16: there is no dtype argument).  Allocates and returns
    (gh, gres or None, dgamma, dbeta, workspace)."""
    B, T, D = x.shape
    _contig(x, "x")
    for t, n in ((gy, "gy"), (res, "res"), (gy2, "gy2")):
        if t is None:
            continue
        _contig(t, n)
        if t.shape != x.shape:
            raise ValueError(f"{name}: {n} must have x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    if gy2 is not None and gy2.dtype != torch.bfloat16:
        raise ValueError(f"{name}: gy2 must be bf16, got {gy2.dtype}")
    gh = torch.empty_like(x)
    gres = None if gres_dtype is None else torch.empty(x.shape, dtype=gres_dtype, device=x.device)
    dg = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty(D, dtype=torch.float32, device=x.device)
    nws = int(_lib.lib().vo_layernorm_bwd_workspace_size(B, T, D)) // 4
    return gh, gres, dg, db, torch.empty(nws, dtype=torch.float32, device=x.device)


def layernorm(x, gamma, beta, res=None, lens=None, out=None, out_dtype=None, eps=1e-5, with_bf16=False):
    """y = LN(x + res) * gamma + beta, rows t >= lens[b] zeroed.  x: (B, T, D).  ``with_bf16``
    (fp32 y only): returns (y, y16), y16 the bf16 copy of y written in the same pass
    (vo_layernorm_dual) for the next conv to read."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, T, D = x.shape
    out, out16 = _ln_fwd("layernorm", x, res, out_dtype or x.dtype, with_bf16, out)
    rdt = vo_dtype(res) if res is not None else vo_dtype(x)
    if with_bf16:
        if out.dtype != torch.float32:
            raise ValueError("layernorm: with_bf16 needs an fp32 output")
        _lib.check(_lib.lib().vo_layernorm_dual(
            _ptr(x), vo_dtype(x), _ptr(res), rdt, _ptr(gamma), _ptr(beta), _ptr(lens), B, T, D, eps, _ptr(out),
            _ptr(out16), _stream(x)), "vo_layernorm_dual")
        return out, out16
    _lib.check(_lib.lib().vo_layernorm(
        _ptr(x), vo_dtype(x), _ptr(res), rdt, _ptr(gamma), _ptr(beta), _ptr(lens), B, T, D, eps, _ptr(out),
        vo_dtype(out), _stream(x)), "vo_layernorm")
    return out


def layernorm_bwd(x, gy, gamma, res=None, lens=None, eps=1e-5):
    """Backward of ``layernorm``: (gh, dgamma, dbeta); gh = dL/d(x + res) in x's dtype."""
    B, T, D = x.shape
    if res is not None and res.dtype != x.dtype:
        raise ValueError("layernorm_bwd: res must match x in shape and dtype")
    gh, _, dg, db, ws = _ln_bwd("layernorm_bwd", x, gy, res)
    _lib.check(_lib.lib().vo_layernorm_bwd(
        _ptr(x), _ptr(res), vo_dtype(x), _ptr(gy), vo_dtype(gy), _ptr(gamma), _ptr(lens), B, T, D, eps, _ptr(gh),
        _ptr(dg), _ptr(db), _ptr(ws), _stream(x)), "vo_layernorm_bwd")
    return gh, dg, db


def layernorm_bwd_ex(x, gy, gamma, res, lens=None, gy2=None, eps=1e-5):
    """Backward of ``layernorm(x, ..., res=res, out_dtype=float32, with_bf16=True)`` with a bf16 x and an
    fp32 res (the training decoder's fp32 residual stream): gy (fp32 or bf16) the gradient of y, gy2
    (bf16, optional) that of the y16 copy -- added in the kernel.  Returns (gh in x's dtype, gh32 =
    the same gradient in fp32 for res, dgamma, dbeta) (vo_layernorm_bwd_ex)."""
    B, T, D = x.shape
    if x.dtype != torch.bfloat16 or res.dtype != torch.float32:
        raise ValueError("layernorm_bwd_ex: bf16 x, fp32 res, gy of x's shape")
    gh, gh32, dg, db, ws = _ln_bwd("layernorm_bwd_ex", x, gy, res, gy2, torch.float32)
    _lib.check(_lib.lib().vo_layernorm_bwd_ex(
        _ptr(x), vo_dtype(x), _ptr(res), vo_dtype(res), _ptr(gy), vo_dtype(gy), _ptr(gy2), _ptr(gamma), _ptr(lens),
        B, T, D, eps, _ptr(gh), _ptr(gh32), _ptr(dg), _ptr(db), _ptr(ws), _stream(x)), "vo_layernorm_bwd_ex")
    return gh, gh32, dg, db


def layernorm_drop(x, gamma, beta, res, p, seed, salt, lens=None, with_bf16=False, eps=1e-5):
    """y = LN(dropout_p(x) + res) * gamma + beta, pad rows zeroed (vo_layernorm_drop): the dropout mask is
    vo_dropout's for the same (seed, salt) on x.  y in res's dtype; with_bf16 (fp32 y): returns (y, y16)."""
    B, T, D = x.shape
    y, y16 = _ln_fwd("layernorm_drop", x, res, res.dtype, with_bf16)
    _lib.check(_lib.lib().vo_layernorm_drop(
        _ptr(x), vo_dtype(x), _ptr(res), vo_dtype(res), _ptr(gamma), _ptr(beta), _ptr(lens), B, T, D, eps, _ptr(y),
        vo_dtype(y), _ptr(y16), float(p), _ptr(seed), int(salt), _stream(x)), "vo_layernorm_drop")
    return (y, y16) if with_bf16 else y


def layernorm_bwd_drop(x, gy, gamma, res, p, seed, salt, lens=None, gy2=None, eps=1e-5):
    """Backward of ``layernorm_drop``: (gh = dL/dx through the mask in x's dtype, gres = dL/dres in res's dtype,
    dgamma, dbeta); gy2 (bf16, optional): the gradient of the y16 copy, added in the kernel."""
    B, T, D = x.shape
    gh, gres, dg, db, ws = _ln_bwd("layernorm_bwd_drop", x, gy, res, gy2, res.dtype)
    _lib.check(_lib.lib().vo_layernorm_bwd_drop(
        _ptr(x), vo_dtype(x), _ptr(res), vo_dtype(res), _ptr(gy), vo_dtype(gy), _ptr(gy2), _ptr(gamma), _ptr(lens),
        B, T, D, eps, float(p), _ptr(seed), int(salt), _ptr(gh), _ptr(gres), _ptr(dg), _ptr(db), _ptr(ws),
        _stream(x)), "vo_layernorm_bwd_drop")
    return gh, gres, dg, db


# ----------------------------------------------------------------------------- attention

def attention(qkv, lens, n_head, out=None, with_lse=False):
    """qkv (B, L, 3D) -> (B, L, D); keys t >= lens[b] masked.  with_lse: also the row log-sum-exp
    (B, H, L) fp32 that attention_bwd(..., lse=) consumes (vo_attention_lse)."""
    _contig(qkv, "qkv")
    B, L, D3 = qkv.shape
    D = D3 // 3
    dk = D // n_head
    out = out if out is not None else torch.empty((B, L, D), dtype=qkv.dtype, device=qkv.device)
    scale = 1.0 / float(dk) ** 0.5
    if with_lse:
        lse = torch.empty((B, n_head, L), dtype=torch.float32, device=qkv.device)
        _lib.check(_lib.lib().vo_attention_lse(_ptr(qkv), vo_dtype(qkv), _ptr(lens), B, L, n_head, dk,
                                               scale, _ptr(out), _ptr(lse), _stream(qkv)), "vo_attention_lse")
        return out, lse
    _lib.check(_lib.lib().vo_attention(_ptr(qkv), vo_dtype(qkv), _ptr(lens), B, L, n_head, dk,
                                       scale, _ptr(out), _stream(qkv)), "vo_attention")
    return out


def attention_bwd(qkv, out, dout, lens, n_head, lse=None):
    """Backward of ``attention``: dqkv (B, L, 3D) in qkv's dtype from the forward output and its
    gradient (flash-style recomputation, vo_attention_bwd); with the forward's row log-sum-exp (lse,
    attention(..., with_lse=True)) the bf16 path skips rebuilding it (vo_attention_bwd_lse)."""
    for t, n in ((qkv, "qkv"), (out, "out"), (dout, "dout")):
        _contig(t, n)
    B, L, D3 = qkv.shape
    D = D3 // 3
    if out.shape != (B, L, D) or dout.shape != (B, L, D):
        raise ValueError("attention_bwd: out / dout must be (B, L, D)")
    if out.dtype != qkv.dtype or dout.dtype != qkv.dtype:
        raise ValueError("attention_bwd: qkv, out and dout must share a dtype")
    dk = D // n_head
    L_ = _lib.lib()
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(int(L_.vo_attention_bwd_workspace_size(B, L, n_head)) // 4, dtype=torch.float32,
                     device=qkv.device)
    if lse is not None:
        if lse.shape != (B, n_head, L) or lse.dtype != torch.float32 or not lse.is_contiguous():
            raise ValueError("attention_bwd: lse must be the forward's (B, H, L) fp32 row log-sum-exp")
        _lib.check(L_.vo_attention_bwd_lse(_ptr(qkv), _ptr(out), _ptr(dout), vo_dtype(qkv), _ptr(lens), B, L, n_head,
                                           dk, 1.0 / float(dk) ** 0.5, _ptr(lse), _ptr(dqkv), _ptr(ws),
                                           _stream(qkv)), "vo_attention_bwd_lse")
        return dqkv
    _lib.check(L_.vo_attention_bwd(_ptr(qkv), _ptr(out), _ptr(dout), vo_dtype(qkv), _ptr(lens), B, L, n_head, dk,
                                   1.0 / float(dk) ** 0.5, _ptr(dqkv), _ptr(ws), _stream(qkv)),
               "vo_attention_bwd")
    return dqkv


# ----------------------------------------------------------------------------- length regulator

def lr_lengths(dur):
    """(B, T) float durations -> (mel_len int64 (B,), mel_len int32 (B,))."""
    dur = _contig(dur.float(), "dur")
    B, T = dur.shape
    m64 = torch.empty(B, dtype=torch.int64, device=dur.device)
    m32 = torch.empty(B, dtype=torch.int32, device=dur.device)
    _lib.check(_lib.lib().vo_lr_lengths(_ptr(dur), B, T, _ptr(m64), _ptr(m32), _stream(dur)),
               "vo_lr_lengths")
    return m64, m32


def length_regulate(x, dur, max_len, out_dtype=None, want_index=False):
    """x (B, T_src, D), dur (B, T_src) float -> (out (B, max_len, D), mel_len int64, index)."""
    _contig(x, "x")
    dur = _contig(dur.float(), "dur")
    B, T, D = x.shape
    out = torch.empty((B, max_len, D), dtype=out_dtype or x.dtype, device=x.device)
    mel_len = torch.empty(B, dtype=torch.int64, device=x.device)
    index = torch.empty((B, max_len), dtype=torch.int32, device=x.device) if want_index else None
    _lib.check(_lib.lib().vo_length_regulate(_ptr(x), vo_dtype(x), _ptr(dur), B, T, D, max_len,
                                             _ptr(out), vo_dtype(out), _ptr(mel_len), _ptr(index),
                                             _stream(x)), "vo_length_regulate")
    return out, mel_len, index


def length_regulate_bwd(go, dur, T_src, out_dtype=torch.float32):
    """Backward of ``length_regulate``: go (B, max_len, D) -> gx (B, T_src, D)."""
    _contig(go, "go")
    dur = _contig(dur.float(), "dur")
    B, max_len, D = go.shape
    gx = torch.empty((B, T_src, D), dtype=out_dtype, device=go.device)
    _lib.check(_lib.lib().vo_length_regulate_bwd(_ptr(go), vo_dtype(go), _ptr(dur), B, T_src, D, max_len, _ptr(gx),
                                                 vo_dtype(gx), _stream(go)), "vo_length_regulate_bwd")
    return gx


# ----------------------------------------------------------------------------- variance heads

def _is_number(c):
    return isinstance(c, (int, float, np.integer, np.floating))


def control_view(control, B, T, device=None):
    """A per-token control as vo_variance_head_ctl takes it: ``(c, n_control, stride_b, stride_t)`` with ``c`` an
    fp32 tensor whose first element is the multiplier of token (0, 0), the strides (in elements, 0 = broadcast) of
    ``c.expand(B, T)`` and ``n_control`` the number of floats from that element to the end of what the view reaches.

    ``control`` is whatever ``torch.broadcast_to(control, (B, T))`` accepts: 0-d, (1,), (T,), (1, T), (B, 1) or
    (B, T), contiguous or not (nothing is materialised); any other shape raises ValueError.  Host only for an fp32
    tensor: no GPU call is made and the values are never read.  Integer, fp64 and bf16 tensors, numpy arrays and
    sequences are converted to fp32 on ``device`` (the activations' device) -- a copy on the current stream, so
    such a call cannot be captured in a graph; an fp64 control is thereby rounded to fp32, where the reference
    would promote its predictions to fp64.  A CUDA tensor on another device than ``device`` raises ValueError."""
    if not isinstance(control, torch.Tensor):
        control = torch.as_tensor(np.asarray(control))
    device = control.device if device is None else torch.device(device)
    if control.is_cuda and control.device != device:
        raise ValueError(f"control is on {control.device}, the activations on {device}")
    try:
        if control.numel() == 0:
            raise RuntimeError("empty")
        control.expand(B, T)
    except RuntimeError:
        raise ValueError(f"control of shape {tuple(control.shape)} does not broadcast to (B, T) = ({B}, {T})") from None
    if control.dtype != torch.float32 or control.device != device:
        control = control.to(device=device, dtype=torch.float32)
    sb, st = control.expand(B, T).stride()
    return control, (B - 1) * sb + (T - 1) * st + 1, sb, st


def _head_launch(d, h, control, B, T):
    """vo_variance_head for a Python-number control (already in ``d``), vo_variance_head_ctl for a tensor one."""
    if control is None:
        _lib.check(_lib.lib().vo_variance_head(ctypes.byref(d), _stream(h)), "vo_variance_head")
        return
    c, n, sb, st = control_view(control, B, T, device=h.device)
    _lib.check(_lib.lib().vo_variance_head_ctl(ctypes.byref(d), _ptr(c), n, sb, st, _stream(h)),
               "vo_variance_head_ctl")


def duration_head(h, w, b, lens, d_control=1.0, want_round=True):
    """Duration prediction (+ rounding).  ``d_control``: a Python number, or a per-token control (``control_view``)
    read on the device.  Returns (log_d, d_round)."""
    B, T, D = h.shape
    pred = torch.empty((B, T), dtype=torch.float32, device=h.device)
    dr = torch.empty((B, T), dtype=torch.float32, device=h.device) if want_round else None
    d = _lib.HeadDesc()
    d.kind = HEAD_DURATION
    d.h, d.h_dtype = h.data_ptr(), vo_dtype(h)
    d.w, d.b = w.data_ptr(), float(b)
    d.lens = lens.data_ptr() if lens is not None else None
    d.B, d.T, d.D = B, T, D
    d.pred = pred.data_ptr()
    d.d_round = dr.data_ptr() if dr is not None else None
    tensor_ctl = not _is_number(d_control)
    d.d_control = 1.0 if tensor_ctl else float(d_control)
    d.x_dtype = vo_dtype(h)
    _head_launch(d, h, d_control if tensor_ctl else None, B, T)
    return pred, dr


def energy_head(h, w, b, lens, x, bins, table, target=None, mean=0.0, std=1.0, control=1.0,
                want_index=False):
    """Energy prediction + bucketize + x += table[idx] (in place).  ``control``: a Python number, or a per-token
    control (``control_view``) read on the device; unused when ``target`` is given.  Returns (pred, idx)."""
    B, T, D = h.shape
    _contig(x, "x")
    pred = torch.empty((B, T), dtype=torch.float32, device=h.device)
    idx = torch.empty((B, T), dtype=torch.int32, device=h.device) if want_index else None
    tgt = _contig(target.float(), "target") if target is not None else None
    d = _lib.HeadDesc()
    d.kind = HEAD_ENERGY
    d.h, d.h_dtype = h.data_ptr(), vo_dtype(h)
    d.w, d.b = w.data_ptr(), float(b)
    d.lens = lens.data_ptr() if lens is not None else None
    d.B, d.T, d.D = B, T, D
    d.pred = pred.data_ptr()
    d.target = tgt.data_ptr() if tgt is not None else None
    d.bins, d.n_bins = bins.data_ptr(), bins.numel()
    tensor_ctl = not _is_number(control)
    d.e_mean, d.e_std, d.e_control = float(mean), float(std), 1.0 if tensor_ctl else float(control)
    d.table = table.data_ptr()
    d.x, d.x_dtype = x.data_ptr(), vo_dtype(x)
    d.idx_out = idx.data_ptr() if idx is not None else None
    _head_launch(d, h, control if tensor_ctl else None, B, T)
    return pred, idx


def bucket_embed(x, target, bins, table):
    """Training-side energy embedding: out = x + table[bucketize(target, bins)] (out of place) ->
    (out, idx int32) (vo_bucket_embed; reference modules.py:53-64,101-104 with a target)."""
    _contig(x, "x")
    B, T, D = x.shape
    tgt = _contig(target.float(), "target")
    if tgt.shape != (B, T):
        raise ValueError(f"bucket_embed: target {tuple(tgt.shape)} vs x {tuple(x.shape)}")
    if table.dim() != 2 or table.shape[1] != D or table.dtype != torch.float32 or not table.is_contiguous():
        raise ValueError(f"bucket_embed: table must be a contiguous fp32 (n, {D}) tensor, got "
                         f"{tuple(table.shape)} {table.dtype}")
    out = torch.empty_like(x)
    idx = torch.empty((B, T), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().vo_bucket_embed(_ptr(x), vo_dtype(x), _ptr(tgt), _ptr(bins), bins.numel(), _ptr(table),
                                          table.shape[0], B * T, D, _ptr(out), _ptr(idx), _stream(x)),
               "vo_bucket_embed")
    return out, idx


def embed_bwd(dy, idx, n_table):
    """dtable (n_table, D) fp32 = per-row sums of dy over the tokens of each index (row order)."""
    _contig(dy, "dy")
    D = dy.shape[-1]
    rows = dy.numel() // D
    dt = torch.empty((n_table, D), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().vo_embed_bwd(_ptr(dy), vo_dtype(dy), _ptr(idx), rows, D, n_table, _ptr(dt), _stream(dy)),
               "vo_embed_bwd")
    return dt


# ----------------------------------------------------------------------------- encoder glue

def vfe_stencil(images, conv_params, bn_params, slice_w, out_dtype):
    """images (B, 1, H, W) fp32 -> (B*n, H*slice_w) flattened stencil output."""
    images = _contig(images.float(), "images")
    B, C, H, W = images.shape
    if C != 1:
        raise ValueError("vfe_stencil: gray-scale (1 channel) images only")
    n = W // slice_w
    out = torch.empty((B * n, H * slice_w), dtype=out_dtype, device=images.device)
    _lib.check(_lib.lib().vo_vfe_stencil(_ptr(images), B, H, W, slice_w, n, _ptr(conv_params),
                                         _ptr(bn_params), conv_params.shape[0], _ptr(out),
                                         vo_dtype(out), _stream(images)), "vo_vfe_stencil")
    return out, n


VFE_LDS_MAX = 160 * 1024  # the window bound of vo_vfe_stencil_ex
VFE_MAX_KERNEL = 9
VFE_MAX_H = 32


def vfe_stencil_lds_bytes(H, win_w, kh, kw):
    """LDS bytes ``vfe_stencil_ex`` needs for an H x win_w window (host only: no GPU call)."""
    return int(_lib.lib().vo_vfe_stencil_lds_bytes(int(H), int(win_w), int(kh), int(kw)))


def vfe_stencil_ex(images, conv_params, bn_params, slice_w, stride, kernel_size, out_dtype, out=None):
    """images (B, 1, H, W) fp32 -> (B*n, H*slice_w*stride): the context windows of ``stride`` cells at a
    step of one cell, each through conv_params.shape[0] layers of kh x kw conv, scale / shift, ReLU.
    conv_params [layers][kh*kw + 1], bn_params [layers][2].  n as the reference counts it
    (scripts/model/visual_feature_extractor.py:67).  ``out``: a contiguous (B*n, H*slice_w*stride) tensor of
    ``out_dtype`` to write instead of a new one."""
    images = _contig(images.float(), "images")
    B, C, H, W = images.shape
    if C != 1:
        raise ValueError("vfe_stencil_ex: gray-scale (1 channel) images only")
    kh, kw = kernel_size
    n = max(int((W - (stride // 2) * slice_w * 2) / slice_w), 0)
    _contig(conv_params, "conv_params")
    _contig(bn_params, "bn_params")
    if conv_params.dim() != 2 or conv_params.shape[1] != kh * kw + 1 or bn_params.shape != (conv_params.shape[0], 2) \
            or conv_params.dtype != torch.float32 or bn_params.dtype != torch.float32:
        raise ValueError(f"vfe_stencil_ex: conv_params {tuple(conv_params.shape)} / bn_params {tuple(bn_params.shape)} "
                         f"must be fp32 (layers, {kh * kw + 1}) and (layers, 2)")
    if out is None:
        out = torch.empty((B * n, H * slice_w * stride), dtype=out_dtype, device=images.device)
    elif tuple(out.shape) != (B * n, H * slice_w * stride) or out.dtype != out_dtype or not out.is_contiguous() \
            or out.device != images.device:
        raise ValueError(f"vfe_stencil_ex: out must be a contiguous {(B * n, H * slice_w * stride)} {out_dtype} tensor "
                         f"on {images.device}")
    _lib.check(_lib.lib().vo_vfe_stencil_ex(_ptr(images), B, H, W, slice_w, stride, n, kh, kw, _ptr(conv_params),
                                            _ptr(bn_params), conv_params.shape[0], _ptr(out), vo_dtype(out),
                                            _stream(images)), "vo_vfe_stencil_ex")
    return out, n


def add_pos_class(x, pe=None, cls=None, cls_idx=None, per_token=False):
    """x (B, T, D) += pe[t] + cls[cls_idx[b]] (or cls[cls_idx[b, t]] when per_token), in place."""
    B, T, D = x.shape
    _contig(x, "x")
    if cls_idx is not None:
        cls_idx = _contig(cls_idx.long(), "cls_idx")
    _lib.check(_lib.lib().vo_add_pos_class(_ptr(x), vo_dtype(x), _ptr(pe), _ptr(cls), _ptr(cls_idx),
                                           1 if per_token else 0, B, T, D, _stream(x)),
               "vo_add_pos_class")
    return x


_LENS_DT = {torch.float32: 0, torch.int64: 2, torch.int32: 3}


def mask_from_lengths(lens, max_len, want_mask=True):
    """-> (mask (B, max_len) bool, True = padding; lens int32 (B,))."""
    lens = _contig(lens, "lens")
    if lens.dtype not in _LENS_DT:
        lens = lens.long()
    B = lens.shape[0]
    mask = torch.empty((B, max_len), dtype=torch.bool, device=lens.device) if want_mask else None
    l32 = torch.empty(B, dtype=torch.int32, device=lens.device)
    _lib.check(_lib.lib().vo_mask_from_lengths(_ptr(lens), _LENS_DT[lens.dtype], B, max_len,
                                               _ptr(mask), _ptr(l32), _stream(lens)),
               "vo_mask_from_lengths")
    return mask, l32


# ----------------------------------------------------------------------------- vocoder glue

def conv_post(x, w_kc, bias, slope=0.01, lens=None, lens_scale=1, pcm_scale=None):
    """x (B, T, C) -> tanh(conv(lrelu(x))) (B, T) fp32; w_kc (K, C) fp32.
    ``lens`` / ``lens_scale`` (ragged batch, as ``conv1d``): sample t of utterance b is computed from its first
    R_b = clamp(lens[b] * lens_scale, 0, T) rows alone for t < R_b and is exactly 0.0 from R_b on.
    ``pcm_scale`` (e.g. 32768.0): the result as int16 (B, T), clamp(trunc(y * pcm_scale), -32768, 32767) stored by
    the same kernels (vo_conv_post_pcm16: truncation toward zero as numpy's astype("int16"), but saturating where
    that cast wraps; NaN -> 0); a scale that is not finite and positive is refused by the library."""
    _contig(x, "x")
    B, T, C = x.shape
    K = w_kc.shape[0]
    if pcm_scale is not None:
        y = torch.empty((B, T), dtype=torch.int16, device=x.device)
        if lens is not None:
            sc = _check_lens(lens, lens_scale, B, x, "conv_post")
            _lib.check(_lib.lib().vo_conv_post_pcm16_lens(_ptr(x), vo_dtype(x), _ptr(w_kc), float(bias), B, T, C, K,
                                                          float(slope), float(pcm_scale), _ptr(y), _stream(x),
                                                          _ptr(lens), sc), "vo_conv_post_pcm16_lens")
            return y
        _lib.check(_lib.lib().vo_conv_post_pcm16(_ptr(x), vo_dtype(x), _ptr(w_kc), float(bias), B, T, C, K,
                                                 float(slope), float(pcm_scale), _ptr(y), _stream(x)),
                   "vo_conv_post_pcm16")
        return y
    y = torch.empty((B, T), dtype=torch.float32, device=x.device)
    if lens is not None:
        sc = _check_lens(lens, lens_scale, B, x, "conv_post")
        _lib.check(_lib.lib().vo_conv_post_lens(_ptr(x), vo_dtype(x), _ptr(w_kc), float(bias), B, T, C, K,
                                                float(slope), _ptr(y), _stream(x), _ptr(lens), sc), "vo_conv_post_lens")
        return y
    _lib.check(_lib.lib().vo_conv_post(_ptr(x), vo_dtype(x), _ptr(w_kc), float(bias), B, T, C, K,
                                       float(slope), _ptr(y), _stream(x)), "vo_conv_post")
    return y


def transpose_bct(x, out_dtype, ldy=None):
    """(B, C, T) fp32 -> (B, T, ldy) channels-last with zero channel padding."""
    x = _contig(x.float(), "x")
    B, C, T = x.shape
    ldy = ldy or C
    y = torch.empty((B, T, ldy), dtype=out_dtype, device=x.device)
    _lib.check(_lib.lib().vo_transpose_bct(_ptr(x), B, C, T, _ptr(y), vo_dtype(y), ldy, _stream(x)),
               "vo_transpose_bct")
    return y


# ----------------------------------------------------------------------------- fused ResBlock pair

def pack_frag(w_packed):
    """[K][C][C] bf16 conv pack (C = 64 / 128) -> the fragment order of the pair kernel (vo_pack_frag)."""
    _contig(w_packed, "w_packed")
    if (w_packed.dtype != torch.bfloat16 or w_packed.dim() != 3 or w_packed.shape[1] != w_packed.shape[2]
            or w_packed.shape[1] not in (64, 128)):
        raise ValueError("pack_frag: a [K][C][C] bf16 pack, C = 64 / 128")
    out = torch.empty_like(w_packed)
    _lib.check(_lib.lib().vo_pack_frag(_ptr(w_packed), _ptr(out), w_packed.shape[1], w_packed.shape[0],
                                       _stream(w_packed)), "vo_pack_frag")
    return out


def resblock_pair(x, w1, b1, w2, b2, K, dil, slope=0.1, out=None, out_scale=1.0, acc=None, tag=None, frag=False,
                  lens=None, lens_scale=1):
    """y = (x + c2(lrelu(c1_dil(lrelu(x))))) * out_scale (+ acc); x (B, T, C) bf16, C in {32, 64, 128}.
    frag: w1 / w2 are pack_frag packs (C = 64 / 128, K = 7 / 11; vo_resblock_pair_frag).
    ``lens`` / ``lens_scale`` (ragged batch, as ``conv1d``; K = 7 / 11): rows past R_b read as zero -- x, acc and the
    c1 output held on chip -- and rows >= R_b of ``out`` are not written.  The timer's FLOPs stay those of the
    padded shape."""
    _contig(x, "x")
    B, T, C = x.shape
    if x.dtype != torch.bfloat16 or w1.dtype != torch.bfloat16 or w2.dtype != torch.bfloat16:
        raise TypeError("resblock_pair: bf16 activations and packed bf16 weights")
    out = out if out is not None else torch.empty_like(x)
    if acc is not None and (acc.shape != x.shape or acc.dtype != x.dtype):
        raise ValueError("resblock_pair: acc must match x")
    timer = profiling.active()
    ev = timer.start() if (tag is not None and timer is not None and timer.watching(tag)) else None
    name = ("vo_resblock_pair_frag" if frag else "vo_resblock_pair") + ("_lens" if lens is not None else "")
    fn = getattr(_lib.lib(), name)
    rag = () if lens is None else (_ptr(lens), _check_lens(lens, lens_scale, B, x, "resblock_pair"))
    _lib.check(fn(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(out), _ptr(acc),
                  B, T, C, K, dil, float(slope), float(out_scale), _stream(x), *rag), name)
    if ev is not None:
        flops = 2.0 * 2.0 * B * T * C * C * K
        nbytes = 2.0 * x.numel() * 2 + (x.numel() * 2 if acc is not None else 0) + 2 * w1.numel() * 2
        name = "mrf_prw_kernel" if (C in (64, 128) and K in (7, 11)) else "mrf_pair_kernel"  # vo_pair_rw_try
        timer.stop(tag, ev, flops, nbytes, kernel=f"{name}<C={C}, ...>")
    return out


VO_NOT_HANDLED = -2  # include/vonoma.h


def _resblock_block(who, K, x, w1s, b1s, w2s, b2s, dils, slope, out, out_scale, acc, tag, lens, lens_scale):
    """The body of ``resblock3`` (K = 3: vo_resblock3) and ``resblock_k`` (vo_resblockk, which takes K and may answer
    VO_NOT_HANDLED -> None); ``who`` names the caller in the errors."""
    whole = who == "resblock_k"
    _contig(x, "x")
    B, T, C = x.shape
    if x.dtype != torch.bfloat16 or any(w.dtype != torch.bfloat16 for w in list(w1s) + list(w2s)):
        raise TypeError(f"{who}: bf16 activations and packed bf16 weights")
    if not (len(w1s) == len(b1s) == len(w2s) == len(b2s) == len(dils) == 3):
        raise ValueError(f"{who}: three stages")
    if whole and any(tuple(w.shape) != (K, C, C) for w in list(w1s) + list(w2s)):
        raise ValueError(f"{who}: weights must be [K][C][C] packs")
    out = out if out is not None else torch.empty_like(x)
    if acc is not None and (acc.shape != x.shape or acc.dtype != x.dtype):
        raise ValueError(f"{who}: acc must match x")
    arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
    dil = (ctypes.c_int * 3)(*[int(d) for d in dils])
    timer = profiling.active()
    ev = timer.start() if (tag is not None and timer is not None and timer.watching(tag)) else None
    name = ("vo_resblockk" if whole else "vo_resblock3") + ("" if lens is None else "_lens")
    rag = () if lens is None else (_ptr(lens), _check_lens(lens, lens_scale, B, x, who))
    kk = (int(K),) if whole else ()
    rc = getattr(_lib.lib(), name)(_ptr(x), arr(w1s), arr(b1s), arr(w2s), arr(b2s), *kk, dil, _ptr(out), _ptr(acc),
                                   B, T, C, float(slope), float(out_scale), _stream(x), *rag)
    if whole and rc == VO_NOT_HANDLED:  # nothing ran; the start event (if any) is dropped unpaired
        return None
    _lib.check(rc, name)
    if ev is not None:
        flops = 3 * 2.0 * 2.0 * B * T * C * C * K
        nbytes = 2.0 * x.numel() * 2 + (x.numel() * 2 if acc is not None else 0) + 6 * w1s[0].numel() * 2
        if whole:  # booked as the three pair launches it stands for (profiling.py: launch units)
            timer.stop(tag, ev, flops, nbytes, kernel=f"mrf_pbk_kernel<K={K}, ...>", launches=3)
        else:
            timer.stop(tag, ev, flops, nbytes, kernel=f"mrf_rb3_kernel<C={C}, ...>")
    return out


def resblock3(x, w1s, b1s, w2s, b2s, dils, slope=0.1, out=None, out_scale=1.0, acc=None, tag=None, lens=None,
              lens_scale=1):
    """A whole K = 3 ResBlock1 (three (c1_d, c2) pairs) in one launch (vo_resblock3):
    y = x_3 * out_scale (+ acc); x (B, T, C) bf16, C in {32, 64, 128}; w1s / w2s: three packed
    [3][C][C] bf16 weights each, b1s / b2s three fp32 biases, dils the three dilations.
    ``lens`` / ``lens_scale`` (ragged batch, as ``conv1d``): rows past R_b read as zero -- x, acc and the on-chip
    T1, x_1, x_2 -- and rows >= R_b of ``out`` are not written.  The timer's FLOPs stay those of the padded shape."""
    return _resblock_block("resblock3", 3, x, w1s, b1s, w2s, b2s, dils, slope, out, out_scale, acc, tag, lens,
                           lens_scale)


def resblock_k_tile_rows(K):
    """Output rows per tile of the whole-block kernel for kernel size K (0: none) -- its tests' edge shapes."""
    return int(_lib.lib().vo_resblockk_tile_rows(int(K)))


def resblock_pair_tile_rows(C, K, dil=1, frag=False):
    """Output rows per tile of the kernel ``resblock_pair`` (``frag``: with pack_frag weights) would launch now for
    a dense call of that shape, vo_tune knobs included (0: a refused shape) -- its tests' edge shapes.  Host only."""
    return int(_lib.lib().vo_resblock_pair_tile_rows(int(C), int(K), int(dil), 1 if frag else 0))


def resblock3_tile_rows(C, dils=(1, 3, 5)):
    """Output rows per tile of the kernel ``resblock3`` would launch now for a dense call with these three dilations,
    vo_tune knobs included (0: a refused shape) -- its tests' edge shapes.  Host only."""
    if len(dils) != 3:
        raise ValueError("resblock3_tile_rows: three dilations")
    dil = (ctypes.c_int * 3)(*[int(d) for d in dils])
    return int(_lib.lib().vo_resblock3_tile_rows(int(C), dil))


def resblock_k(x, w1s, b1s, w2s, b2s, K, dils, slope=0.1, out=None, out_scale=1.0, acc=None, tag=None, lens=None,
               lens_scale=1):
    """A whole K = 7 / 11 ResBlock1 (three (c1_d, c2) pairs) in one launch (vo_resblockk):
    y = x_3 * out_scale (+ acc); x (B, T, C) bf16; w1s / w2s: three packed [K][C][C] bf16 weights each, b1s / b2s
    three fp32 biases, dils the three dilations.  x_1, x_2 and the c1 outputs stay on chip.
    Returns ``out``, or None when no whole-block kernel covers the call (it exists for C = 32, K = 7 / 11, dilations
    (1, 3, 5), and with ``acc`` only when 1 / out_scale is a bf16 value): nothing was launched and the caller runs
    three ``resblock_pair`` launches.
    ``lens`` / ``lens_scale`` (ragged batch, as ``conv1d``): rows past R_b read as zero -- x, acc and the on-chip
    T1, x_1, x_2 -- and rows >= R_b of ``out`` are not written.  The timer's FLOPs stay those of the padded shape;
    under ``tag`` the launch counts as three launch units (the pairs it replaces), with the block's whole FLOPs
    and algorithmic bytes."""
    return _resblock_block("resblock_k", K, x, w1s, b1s, w2s, b2s, dils, slope, out, out_scale, acc, tag, lens,
                           lens_scale)


# ----------------------------------------------------------------------------- mel / STFT

def stft_mel(wav, window, fb, n_fft=1024, hop=256, n_mels=80, log_floor=1e-5):
    """wav (B, N) fp32 -> (log-mel (B, n_mels, 1 + N // hop), energy (B, 1 + N // hop))."""
    _contig(wav, "wav")
    B, N = wav.shape
    F = 1 + N // hop
    mel = torch.empty((B, n_mels, F), dtype=torch.float32, device=wav.device)
    energy = torch.empty((B, F), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().vo_stft_mel(_ptr(wav), B, N, _ptr(window), _ptr(fb), n_fft, hop, n_mels,
                                      float(log_floor), _ptr(mel), _ptr(energy), _stream(wav)),
               "vo_stft_mel")
    return mel, energy


def stft_mel_ex(wav, window, fb, n_fft=1024, hop=256, n_mels=80, pad=None, mag_eps=0.0, clip=False,
                log_floor=1e-5):
    """General framing (vo_stft_mel_ex): wav (B, N) fp32 -> log-mel (B, n_mels, F),
    F = 1 + (N + 2 pad - n_fft) // hop.  HiFi-GAN training mel: pad=(n_fft-hop)//2, mag_eps=1e-9."""
    _contig(wav, "wav")
    B, N = wav.shape
    pad = n_fft // 2 if pad is None else pad
    F = 1 + (N + 2 * pad - n_fft) // hop
    mel = torch.empty((B, n_mels, F), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().vo_stft_mel_ex(_ptr(wav), B, N, _ptr(window), _ptr(fb), n_fft, hop, n_mels, pad,
                                         float(mag_eps), int(bool(clip)), float(log_floor), _ptr(mel), None, None,
                                         _stream(wav)), "vo_stft_mel_ex")
    return mel


def stft_mel_frames(n, n_fft=1024, hop=256, pad=None):
    """Frames of an n-sample signal under ``stft_mel_lens`` (vo_stft_mel_frames, host only): 1 + (n + 2 pad - n_fft)
    // hop when n > pad and n + 2 pad >= n_fft, else 0."""
    pad = n_fft // 2 if pad is None else pad
    return int(_lib.lib().vo_stft_mel_frames(int(n), int(n_fft), int(hop), int(pad)))


def _wave_lens32(lens, B, N, ref):
    """``lens`` of ``stft_mel_lens`` -> contiguous int32 (B,) on ``ref``'s device.  A device tensor (int32 / int64) is
    converted on the device and never read on the host (the kernel clamps it to [0, N]); a host sequence is
    validated here."""
    if isinstance(lens, torch.Tensor):
        if lens.dtype not in (torch.int32, torch.int64) or lens.shape != (B,):
            raise ValueError(f"stft_mel_lens: lens must be an int32 / int64 tensor of shape ({B},), got {lens.dtype} "
                             f"{tuple(lens.shape)}")
        if lens.device != ref.device:
            raise ValueError(f"stft_mel_lens: lens is on {lens.device}, the waveform on {ref.device}")
        return lens.to(torch.int32).contiguous()
    host = [int(v) for v in lens]
    if len(host) != B or any(v < 0 or v > N for v in host):
        raise ValueError(f"stft_mel_lens: lens must be {B} sample counts in [0, {N}], got {host}")
    return torch.tensor(host, dtype=torch.int32).to(ref.device)


def _out_f32(t, shape, ref, name):
    """A preallocated fp32 output of ``shape`` on ``ref``'s device, or a new one."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=ref.device)
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != ref.device:
        raise ValueError(f"stft_mel_lens: {name} must be fp32 {tuple(shape)} on {ref.device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return _contig(t, name)


def stft_mel_lens(wav, window, fb, lens, n_fft=1024, hop=256, pad=None, mag_eps=0.0, clip=False, log_floor=1e-5,
                  channels_last=False, want_energy=True, want_fstats=False, mel=None, energy=None, fstats=None):
    """``stft_mel_ex`` of a ragged batch in one launch (vo_stft_mel_lens): wav (B, N) fp32 whose row b holds
    lens[b] samples -> (mel, energy, fstats, frames).  mel is (B, n_mels, F), or (B, F, n_mels) with
    ``channels_last``, F = stft_mel_frames(N); energy (B, F) and fstats (B, F, 2) are None unless wanted (or handed
    in); frames is the device int32 (B,) of per-row frame counts F_b = stft_mel_frames(lens[b]).  Frames f < F_b of
    row b are bit for bit those of the dense call on wav[b:b+1, :lens[b]] (no sample past lens[b] is read), frames
    >= F_b are 0.  ``lens``: int32 / int64 device tensor (never read on the host: the call is graph-capturable and
    a replay follows lengths changed in place), a host sequence of B counts in [0, N], or None (every row is N)."""
    _contig(wav, "wav")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError(f"stft_mel_lens: wav must be fp32 (B, N), got {wav.dtype} {tuple(wav.shape)}")
    B, N = wav.shape
    n_mels = fb.shape[1]
    pad = n_fft // 2 if pad is None else pad
    st = _stream(wav)
    lens32 = None if lens is None else _wave_lens32(lens, B, N, wav)
    F = stft_mel_frames(N, n_fft, hop, pad)  # 0: empty outputs; the entry refuses such an N, nothing is launched
    mel = _out_f32(mel, (B, F, n_mels) if channels_last else (B, n_mels, F), wav, "mel")
    if want_energy or energy is not None:
        energy = _out_f32(energy, (B, F), wav, "energy")
    if want_fstats or fstats is not None:
        fstats = _out_f32(fstats, (B, F, 2), wav, "fstats")
    frames = torch.empty(B, dtype=torch.int32, device=wav.device)
    _lib.check(_lib.lib().vo_stft_mel_lens(_ptr(wav), B, N, _ptr(window), _ptr(fb), n_fft, hop, n_mels, pad,
                                           float(mag_eps), int(bool(clip)), float(log_floor), _ptr(mel),
                                           _ptr(energy), _ptr(fstats), _ptr(lens32), _ptr(frames),
                                           int(channels_last), st), "vo_stft_mel_lens")
    return mel, energy, fstats, frames


def stft_mel_bwd(wav, window, fb, gmel, n_fft=1024, hop=256, pad=None, mag_eps=1e-9, log_floor=1e-5):
    """Backward of ``stft_mel_ex`` (clip off): gmel (B, n_mels, F) = dL/dlogmel -> dL/dwav (B, N) fp32."""
    _contig(wav, "wav")
    _contig(gmel, "gmel")
    B, N = wav.shape
    n_mels = fb.shape[1]
    pad = n_fft // 2 if pad is None else pad
    F = 1 + (N + 2 * pad - n_fft) // hop
    if gmel.shape != (B, n_mels, F) or gmel.dtype != torch.float32 or wav.dtype != torch.float32:
        raise ValueError(f"stft_mel_bwd: gmel {tuple(gmel.shape)} {gmel.dtype} vs ({B}, {n_mels}, {F}) fp32")
    L = _lib.lib()
    dwav = torch.empty_like(wav)
    ws = torch.empty(int(L.vo_stft_mel_bwd_workspace_size(B, N, n_fft, hop, pad)) // 4, dtype=torch.float32,
                     device=wav.device)
    _lib.check(L.vo_stft_mel_bwd(_ptr(wav), B, N, _ptr(window), _ptr(fb), n_fft, hop, n_mels, pad, float(mag_eps),
                                 float(log_floor), _ptr(gmel), _ptr(dwav), _ptr(ws), _stream(wav)), "vo_stft_mel_bwd")
    return dwav


def stft_mag(wav, window, n_fft, hop, eps=1e-7):
    """torch.stft(center=True, reflect, onesided) magnitude sqrt(max(|X|^2, eps)) of wav (B, N) fp32
    with ``window`` zero-padded to n_fft -> (B, 1 + N // hop, n_fft // 2 + 1)."""
    _contig(wav, "wav")
    B, N = wav.shape
    if window.numel() != n_fft:
        raise ValueError("stft_mag: window must be zero-padded to n_fft")
    mag = torch.empty((B, 1 + N // hop, n_fft // 2 + 1), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().vo_stft_mag(_ptr(wav), B, N, _ptr(window), n_fft, hop, float(eps), _ptr(mag), _stream(wav)),
               "vo_stft_mag")
    return mag


def stft_mag_bwd(wav, window, gmag, n_fft, hop, eps=1e-7):
    """Backward of ``stft_mag``: gmag (B, F, bins) -> dL/dwav (B, N) fp32."""
    _contig(wav, "wav")
    _contig(gmag, "gmag")
    B, N = wav.shape
    if gmag.shape != (B, 1 + N // hop, n_fft // 2 + 1):
        raise ValueError("stft_mag_bwd: gmag shape")
    L = _lib.lib()
    dwav = torch.empty_like(wav)
    ws = torch.empty(int(L.vo_stft_mag_bwd_workspace_size(B, N, n_fft, hop)) // 4, dtype=torch.float32,
                     device=wav.device)
    _lib.check(L.vo_stft_mag_bwd(_ptr(wav), B, N, _ptr(window), n_fft, hop, float(eps), _ptr(gmag), _ptr(dwav),
                                 _ptr(ws), _stream(wav)), "vo_stft_mag_bwd")
    return dwav


def stft_loss_sums(xm, ym):
    """(sum (y - x)^2, sum y^2, sum |log y - log x|) over two magnitude tensors -> fp32 (3,)."""
    _contig(xm, "xm")
    _contig(ym, "ym")
    if xm.shape != ym.shape:
        raise ValueError("stft_loss_sums: shape mismatch")
    out = torch.empty(3, dtype=torch.float32, device=xm.device)
    ws = torch.empty(3 * 512, dtype=torch.float32, device=xm.device)
    _lib.check(_lib.lib().vo_stft_loss(_ptr(xm), _ptr(ym), xm.numel(), _ptr(out), _ptr(ws), _stream(xm)),
               "vo_stft_loss")
    return out


def stft_loss_grad(xm, ym, sums, w):
    """d(w[0] * spectral convergence + w[1] * log-magnitude L1)/dxm; w: fp32 (2,) on the device."""
    w = w.float().contiguous()
    gx = torch.empty_like(xm)
    _lib.check(_lib.lib().vo_stft_loss_grad(_ptr(xm), _ptr(ym), xm.numel(), _ptr(sums), _ptr(w), _ptr(gx),
                                            _stream(xm)), "vo_stft_loss_grad")
    return gx


# ----------------------------------------------------------------------------- training BatchNorm / glyph conv

def _rows(x):
    """Channels-last view as (M, C); a single-channel map (N, 1, H, W) is M = every pixel, C = 1."""
    _contig(x, "x")
    C = x.shape[-1] if x.dim() != 4 else x.shape[1]
    if x.dim() == 4 and C != 1:
        raise ValueError("bn: 4-d input must be single-channel (N, 1, H, W)")
    return x.numel() // C, C


BN_ROUTE_FIELDS = ("route", "V", "CV", "RL", "RB", "nb", "apply_blocks", "CT")
BN_SCALAR, BN_VEC, BN_FLAT = 0, 1, 2  # route


def bn_route(M, C, x_dtype, dy_dtype=None, x=None, dy=None, out=None):
    """The kernels ``bn_train_fwd`` (dy_dtype None) or ``bn_bwd`` would launch for an (M, C) input, as a dict over
    BN_ROUTE_FIELDS (vo_bn_route in include/vonoma.h: the routing the launches themselves run).  x_dtype /
    dy_dtype: torch dtypes.  x, dy, out: the call's tensors or addresses, only their alignment is looked at
    (None: aligned).  Host only: nothing is launched and no tensor is read."""
    def addr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    rec = (ctypes.c_int32 * len(BN_ROUTE_FIELDS))()
    n = _lib.lib().vo_bn_route(int(M), int(C), vo_dtype(x_dtype), -1 if dy_dtype is None else vo_dtype(dy_dtype),
                               addr(x), addr(dy), addr(out), rec, len(BN_ROUTE_FIELDS))
    if n != len(BN_ROUTE_FIELDS):
        _lib.check(n if n < 0 else -1, "vo_bn_route")
    return dict(zip(BN_ROUTE_FIELDS, (int(v) for v in rec)))


def bn_train_fwd(x, gamma, beta, eps, momentum, running_mean=None, running_var=None, num_batches=None):
    """BatchNorm with batch statistics over channels-last x (..., C) or (N, 1, H, W) in fp32 / bf16:
    (y in x's dtype, mean_rstd (2C) fp32); running stats / num_batches updated in place when given."""
    M, C = _rows(x)
    L = _lib.lib()
    y = torch.empty_like(x)
    mr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.vo_bn_workspace_size(M, C)) // 4, dtype=torch.float32, device=x.device)
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()):
            raise ValueError(f"bn_train_fwd: {n} must be contiguous fp32 of {C}")
    if num_batches is not None and num_batches.dtype != torch.int64:
        raise ValueError("bn_train_fwd: num_batches must be int64")
    _lib.check(L.vo_bn_train_fwd(_ptr(x), vo_dtype(x), M, C, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                 _ptr(running_mean), _ptr(running_var), _ptr(num_batches), _ptr(mr), _ptr(ws), _ptr(y),
                                 _stream(x)), "vo_bn_train_fwd")
    return y, mr


def dropout(x, p, seed, salt=0, out=None):
    """Training dropout (vo_dropout): x / (1 - p) where hash(seed, salt, i) >= p 2^32, else 0; ``seed`` a
    device int64 tensor (one element), ``salt`` the dropout site.  The same call on a gradient with the
    same seed and salt is the backward."""
    _contig(x, "x")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dropout: fp32 / bf16")
    if seed.dtype != torch.int64 or seed.numel() < 1 or seed.device != x.device:
        raise ValueError("dropout: seed must be an int64 tensor on x's device")
    out = out if out is not None else torch.empty_like(x)
    _lib.check(_lib.lib().vo_dropout(_ptr(x), vo_dtype(x), x.numel(), float(p), _ptr(seed), int(salt) & 0xFFFFFFFF,
                                     _ptr(out), _stream(x)), "vo_dropout")
    return out


def bn_bwd(x, gy, gamma, mean_rstd):
    """Backward of ``bn_train_fwd``: (dx in x's dtype, dgamma, dbeta) fp32."""
    M, C = _rows(x)
    _contig(gy, "gy")
    if gy.shape != x.shape:
        raise ValueError("bn_bwd: gy shape mismatch")
    L = _lib.lib()
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.vo_bn_workspace_size(M, C)) // 4, dtype=torch.float32, device=x.device)
    _lib.check(L.vo_bn_bwd(_ptr(x), vo_dtype(x), _ptr(gy), vo_dtype(gy), M, C, _ptr(gamma), _ptr(mean_rstd), _ptr(ws),
                           _ptr(dg), _ptr(db), _ptr(dx), _stream(x)), "vo_bn_bwd")
    return dx, dg, db


def _vfe_shape(x):
    _contig(x, "x")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise ValueError(f"vfe conv: x must be (N, 1, H, W) fp32, got {tuple(x.shape)} {x.dtype}")
    return x.shape[0], x.shape[2], x.shape[3]


def vfe_conv_fwd(x, w10):
    """Conv2d(1, 1, 3, padding=1): x (N, 1, H, W) fp32, w10 = 9 kernel taps (row-major) + bias."""
    N, H, W = _vfe_shape(x)
    y = torch.empty_like(x)
    _lib.check(_lib.lib().vo_vfe_conv_fwd(_ptr(x), N, H, W, _ptr(w10), _ptr(y), _stream(x)), "vo_vfe_conv_fwd")
    return y


def vfe_conv_bwd(x, gy, w10):
    """Backward of ``vfe_conv_fwd``: (dx, dw10)."""
    N, H, W = _vfe_shape(x)
    _contig(gy, "gy")
    if gy.shape != x.shape or gy.dtype != torch.float32:
        raise ValueError("vfe_conv_bwd: gy must match x")
    L = _lib.lib()
    dx = torch.empty_like(x)
    dw = torch.empty(10, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.vo_vfe_conv_workspace_size(N, H, W)) // 4, dtype=torch.float32, device=x.device)
    _lib.check(L.vo_vfe_conv_bwd(_ptr(x), _ptr(gy), N, H, W, _ptr(w10), _ptr(dx), _ptr(dw), _ptr(ws), _stream(x)),
               "vo_vfe_conv_bwd")
    return dx, dw


def _vfe_taps(w, kh, kw, what):
    _contig(w, "w")
    if w.dtype != torch.float32 or w.numel() != kh * kw + 1:
        raise ValueError(f"{what}: w must be {kh * kw + 1} fp32 values ({kh} x {kw} taps + bias), got {tuple(w.shape)}")


def vfe_conv_fwd_ex(x, w, kh, kw):
    """Conv2d(1, 1, (kh, kw), padding ((kh-1)/2, (kw-1)/2)): x (N, 1, H, W) fp32, w = kh*kw taps (row-major) + bias."""
    N, H, W = _vfe_shape(x)
    _vfe_taps(w, kh, kw, "vfe_conv_fwd_ex")
    y = torch.empty_like(x)
    _lib.check(_lib.lib().vo_vfe_conv_fwd_ex(_ptr(x), N, H, W, kh, kw, _ptr(w), _ptr(y), _stream(x)),
               "vo_vfe_conv_fwd_ex")
    return y


def vfe_conv_bwd_ex(x, gy, w, kh, kw):
    """Backward of ``vfe_conv_fwd_ex``: (dx, dw[kh*kw + 1])."""
    N, H, W = _vfe_shape(x)
    _vfe_taps(w, kh, kw, "vfe_conv_bwd_ex")
    _contig(gy, "gy")
    if gy.shape != x.shape or gy.dtype != torch.float32:
        raise ValueError("vfe_conv_bwd_ex: gy must match x")
    L = _lib.lib()
    nbytes = int(L.vo_vfe_conv_workspace_size_ex(N, H, W, kh, kw))
    if nbytes < 0:
        raise ValueError(f"vfe_conv_bwd_ex: {N} x {H} x {W} maps with a {kh} x {kw} kernel unsupported (odd sizes up to 9)")
    dx = torch.empty_like(x)
    dw = torch.empty(kh * kw + 1, dtype=torch.float32, device=x.device)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    _lib.check(L.vo_vfe_conv_bwd_ex(_ptr(x), _ptr(gy), N, H, W, kh, kw, _ptr(w), _ptr(dx), _ptr(dw), _ptr(ws),
                                    _stream(x)), "vo_vfe_conv_bwd_ex")
    return dx, dw


# ----------------------------------------------------------------------------- HiFi-GAN training (C5)

def pack_grouped_weight(w, dtype, groups=1, ci_pad=None, out=None):
    """(Co, Ci/groups, K) fp32 -> dense [K][Co][Ci_pad] block-diagonal (vo_conv1d groups mode).
    ``out``: a buffer of that shape and dtype whose entries outside the diagonal blocks are zero
    (a persistent packed weight): only the blocks are rewritten (vo_pack_grouped_blocks)."""
    w = w.detach().float().contiguous()
    Co, cig, K = w.shape
    Ci = cig * groups
    ci_pad = Ci if ci_pad is None else ci_pad
    if out is not None:
        if tuple(out.shape) != (K, Co, ci_pad) or out.dtype != dtype or not out.is_contiguous():
            raise ValueError(f"pack_grouped_weight: out {tuple(out.shape)} {out.dtype}, "
                             f"expected contiguous {(K, Co, ci_pad)} {dtype}")
        _lib.check(_lib.lib().vo_pack_grouped_blocks(_ptr(w), Co, Ci, K, groups, ci_pad, _ptr(out),
                                                     vo_dtype(dtype), _stream(w)), "vo_pack_grouped_blocks")
        return out
    out = torch.empty((K, Co, ci_pad), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().vo_pack_grouped(_ptr(w), Co, Ci, K, groups, ci_pad, _ptr(out), vo_dtype(dtype),
                                          _stream(w)), "vo_pack_grouped")
    return out


PJ_GATHER, PJ_CONVT = 0, 1
_PJ_FIELDS = ("mode", "swap", "T", "rows", "width", "dst_rows", "ld", "rpg", "cpg", "cig", "K", "tap0", "tstep",
              "src_rows")


def pack_batch(jobs, dtype):
    """Many weight packs in one launch (vo_pack_batch; layouts in include/vonoma.h): jobs is a list of
    (src fp32 contiguous, dst contiguous tensor of ``dtype``, {field: int}[, element offset of the job's
    block in dst]).  Entries of dst a job does not name are left as they are."""
    if not jobs:
        return
    arr = (_lib.PackJob * len(jobs))()
    for e, job in zip(arr, jobs):
        src, dst, f = job[:3]
        off = job[3] if len(job) > 3 else None  # element offset of the job's (0, 0) in dst (a block of it)
        _contig(src, "src")
        _contig(dst, "dst")
        if src.dtype != torch.float32 or dst.dtype != dtype:
            raise ValueError("pack_batch: src must be fp32 and dst the batch dtype")
        rows_total = f["T"] * f["dst_rows"] * f["ld"]
        if off is None and dst.numel() != rows_total:
            raise ValueError(f"pack_batch: dst has {dst.numel()} elements, the job's layout {rows_total}")
        if off is not None:  # the last element the job writes must lie in dst
            last = (off + (f["T"] - 1) * f["dst_rows"] * f["ld"] + (f["rows"] - 1) * f["ld"] +
                    ((f["rows"] - 1) // f["rpg"]) * f["cpg"] + f["width"])
            if off < 0 or last > dst.numel():
                raise ValueError(f"pack_batch: a block at {off} of {dst.numel()} elements ends at {last}")
        e.src, e.dst = src.data_ptr(), dst.data_ptr() + (off or 0) * dst.element_size()
        for k in _PJ_FIELDS:
            setattr(e, k, int(f[k]))
    _lib.check(_lib.lib().vo_pack_batch(len(jobs), ctypes.cast(arr, ctypes.c_void_p), vo_dtype(dtype),
                                        _stream(jobs[0][1])), "vo_pack_batch")


def seq_remap(src, dst_rows, Td, Ss, lo, hi, shift):
    """Rows of a channels-last tensor remapped (vo_seq_remap): returns (dst_rows, C) with row
    r = (n, t) (n = r // Td, t = r % Td) = src row n Ss + t + shift for lo <= t < hi, else 0.
    ``src``: contiguous, its last dim the row."""
    _contig(src, "src")
    C = src.shape[-1]
    rows = src.numel() // C
    dst = torch.empty((dst_rows, C), dtype=src.dtype, device=src.device)
    _lib.check(_lib.lib().vo_seq_remap(_ptr(src), rows, _ptr(dst), dst_rows, C * src.element_size(), Td, Ss, lo, hi,
                                       shift, _stream(src)), "vo_seq_remap")
    return dst


def seq_remap2(jobs):
    """One or two remaps in one launch (vo_seq_remap2): each job a dict(src, dst_rows, Td, Ss, lo, hi,
    shift[, src2, Ss2, shift2]) -> its (dst_rows, C) tensor: row r = (n, t) (n = r // Td, t = r % Td)
    = src row n Ss + t + shift (+ src2 row n Ss2 + t + shift2, added in the dtype) for lo <= t < hi,
    else 0.  Sources contiguous with the same row (C) and dtype, rows of whole 16-byte units."""
    if not 1 <= len(jobs) <= 2:
        raise ValueError("seq_remap2: one or two jobs")
    ref = jobs[0]["src"]
    C = ref.shape[-1]
    arr = (_lib.RemapJob * len(jobs))()
    outs = []
    for i, j in enumerate(jobs):
        src, src2 = j["src"], j.get("src2")
        for t in (src, src2):
            if t is not None:
                _contig(t, "src")
                if t.shape[-1] != C or t.dtype != ref.dtype:
                    raise ValueError("seq_remap2: sources must share the row and dtype")
        dst = torch.empty((j["dst_rows"], C), dtype=ref.dtype, device=ref.device)
        outs.append(dst)
        a = arr[i]
        a.src, a.dst = src.data_ptr(), dst.data_ptr()
        a.src2 = src2.data_ptr() if src2 is not None else None
        a.src_rows = src.numel() // C
        a.src2_rows = src2.numel() // C if src2 is not None else 0
        a.dst_rows, a.Td, a.Ss, a.lo, a.hi, a.shift = j["dst_rows"], j["Td"], j["Ss"], j["lo"], j["hi"], j["shift"]
        a.Ss2, a.shift2 = j.get("Ss2", 0), j.get("shift2", 0)
    _lib.check(_lib.lib().vo_seq_remap2(len(jobs), arr, C * ref.element_size(), vo_dtype(ref), _stream(ref)),
               "vo_seq_remap2")
    return outs


def pack_dgrad_phase(w, groups, S, k_r, J, ci_out, co_in, dtype, out=None):
    """Stride phase k_r of a strided / grouped conv's input gradient: w (Co, Ci/groups, K) -> packed
    [J][ci_out][co_in] (taps k_r + S (J - 1 - t), channel roles swapped per group, zero padding).
    ``out``: a persistent buffer of that shape, zero outside the diagonal blocks (only they are written)."""
    w = w.detach().float().contiguous()
    Co, cig, K = w.shape
    shape = (J, ci_out, co_in)
    if out is not None:
        if tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
            raise ValueError(f"pack_dgrad_phase: out {tuple(out.shape)} {out.dtype}, expected contiguous {shape} {dtype}")
    dst = out if out is not None else torch.empty(shape, dtype=dtype, device=w.device)
    _lib.check(_lib.lib().vo_pack_dgrad_phase(_ptr(w), Co, cig, K, groups, S, k_r, J, ci_out, co_in,
                                              1 if out is not None else 0, _ptr(dst), vo_dtype(dtype), _stream(w)),
               "vo_pack_dgrad_phase")
    return dst


def period_fold(wav, period, dtype):
    """wav (B, T) fp32 -> (B * period, ceil(T / period), 8) channels-last (MPD input)."""
    _contig(wav, "wav")
    B, T = wav.shape
    H = (T + period - 1) // period
    out = torch.empty((B * period, H, 8), dtype=dtype, device=wav.device)
    _lib.check(_lib.lib().vo_period_fold(_ptr(wav), B, T, period, _ptr(out), vo_dtype(dtype), _stream(wav)),
               "vo_period_fold")
    return out


def wav_cl8(wav, dtype):
    """(B, T) fp32 -> (B, T, 8) channels-last, channel 0 = wav (MSD input)."""
    _contig(wav, "wav")
    out = torch.empty(wav.shape + (8,), dtype=dtype, device=wav.device)
    _lib.check(_lib.lib().vo_wav_cl8(_ptr(wav), wav.numel(), _ptr(out), vo_dtype(dtype), _stream(wav)),
               "vo_wav_cl8")
    return out


def avgpool_wav(wav):
    """AvgPool1d(4, 2, padding=2) over (B, T) fp32 -> (B, T // 2 + 1)."""
    _contig(wav, "wav")
    B, T = wav.shape
    out = torch.empty((B, T // 2 + 1), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().vo_avgpool_wav(_ptr(wav), B, T, _ptr(out), _stream(wav)), "vo_avgpool_wav")
    return out


def period_fold_bwd(g, B, T, period):
    """Adjoint of ``period_fold``: g (B * period, H, 8) -> dL/dwav (B, T) fp32."""
    _contig(g, "g")
    H = (T + period - 1) // period
    if g.shape != (B * period, H, 8):
        raise ValueError(f"period_fold_bwd: g {tuple(g.shape)} vs ({B * period}, {H}, 8)")
    gw = torch.empty((B, T), dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().vo_period_fold_bwd(_ptr(g), vo_dtype(g), B, T, period, _ptr(gw), _stream(g)),
               "vo_period_fold_bwd")
    return gw


def _ptr_table(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)


def _wn_check(vs, gs):
    if len(vs) != len(gs):
        raise ValueError("weight_norm: as many g as v")
    for v, g in zip(vs, gs):
        _contig(v, "v")
        _contig(g, "g")
        if v.dtype != torch.float32 or g.dtype != torch.float32:
            raise ValueError("weight_norm: fp32 v and g")
        if g.numel() != v.shape[0] or v.device != vs[0].device:
            raise ValueError(f"weight_norm: g {tuple(g.shape)} vs v {tuple(v.shape)} (one gain per row of dim 0)")
    rows = [v.shape[0] for v in vs]
    lens = [v.numel() // v.shape[0] for v in vs]
    return (ctypes.c_int * len(vs))(*rows), (ctypes.c_int * len(vs))(*lens)


def weight_norm(vs, gs):
    """w_k = g_k * v_k / ||v_k||, norms over every dim but 0 (torch._weight_norm(v, g, 0)), for a list
    of layers in one launch per 24 layers (vo_weight_norm) -> list of w."""
    if not vs:
        return []
    rows, lens = _wn_check(vs, gs)
    ws = [torch.empty_like(v) for v in vs]
    _lib.check(_lib.lib().vo_weight_norm(len(vs), _ptr_table(vs), _ptr_table(gs), _ptr_table(ws), rows, lens,
                                          _stream(vs[0])), "vo_weight_norm")
    return ws


def spectral_norm(Ws, us, vs, power, eps=1e-12):
    """torch.nn.utils.spectral_norm's weight for many layers (vo_spectral_norm): Ws = weight_orig
    (rows, ...) fp32, us / vs the u / v buffers (updated in place when ``power``) -> (w list, the u and
    v copies sigma used, sigma list (1-element tensors))."""
    n = len(Ws)
    if n == 0:
        return [], [], [], []
    arr = (_lib.SnLayer * n)()
    outs = []
    for e, W, u, v in zip(arr, Ws, us, vs):
        for t, name in ((W, "W"), (u, "u"), (v, "v")):
            _contig(t, name)
            if t.dtype != torch.float32:
                raise ValueError(f"spectral_norm: {name} must be fp32")
        rows, L = W.shape[0], W.numel() // W.shape[0]
        if u.numel() != rows or v.numel() != L:
            raise ValueError("spectral_norm: u / v do not match the weight")
        o = dict(u_out=torch.empty_like(u), v_out=torch.empty_like(v), vraw=torch.empty_like(v),
                 s=torch.empty_like(u), sigma=torch.empty(1, dtype=torch.float32, device=W.device),
                 w=torch.empty_like(W))
        outs.append(o)
        e.W, e.u, e.v = W.data_ptr(), u.data_ptr(), v.data_ptr()
        for k in ("u_out", "v_out", "vraw", "s", "sigma", "w"):
            setattr(e, k, o[k].data_ptr())
        e.rows, e.L = rows, L
    _lib.check(_lib.lib().vo_spectral_norm(n, ctypes.cast(arr, ctypes.c_void_p), 1 if power else 0, float(eps),
                                           _stream(Ws[0])), "vo_spectral_norm")
    return [o["w"] for o in outs], [o["u_out"] for o in outs], [o["v_out"] for o in outs], [o["sigma"] for o in outs]


def spectral_norm_bwd(gs, Ws, us, vs, sigmas):
    """Gradients wrt weight_orig of spectral_norm's weights (vo_spectral_norm_bwd): gs / Ws (rows, ...)
    fp32, us / vs / sigmas as the forward used them -> [gW] (gW = g / s - (sum(g W) / s^2) u v^T)."""
    n = len(gs)
    arr = (_lib.SnBwdLayer * n)()
    outs = []
    keep = []
    for e, g, W, u, v, sg in zip(arr, gs, Ws, us, vs, sigmas):
        g = g.float().contiguous()
        for t, name in ((W, "W"), (u, "u"), (v, "v"), (sg, "sigma")):
            _contig(t, name)
        if g.shape != W.shape:
            raise ValueError("spectral_norm_bwd: gradient and weight shapes differ")
        o = torch.empty_like(W)
        outs.append(o)
        keep.append(g)
        e.g, e.W, e.u, e.v, e.sigma, e.gW = g.data_ptr(), W.data_ptr(), u.data_ptr(), v.data_ptr(), sg.data_ptr(), o.data_ptr()
        e.rows, e.L = W.shape[0], W.numel() // W.shape[0]
    L = _lib.lib()
    p = ctypes.cast(arr, ctypes.c_void_p)
    ws = torch.empty(max(1, int(L.vo_spectral_norm_bwd_workspace_size(n, p)) // 4), dtype=torch.float32,
                     device=Ws[0].device)
    _lib.check(L.vo_spectral_norm_bwd(n, p, _ptr(ws), _stream(Ws[0])), "vo_spectral_norm_bwd")
    return outs


def weight_norm_bwd(vs, gs, dws):
    """Backward of ``weight_norm``: lists of dL/dw -> (dL/dv list, dL/dg list)."""
    if not vs:
        return [], []
    rows, lens = _wn_check(vs, gs)
    for v, d in zip(vs, dws):
        _contig(d, "dw")
        if d.shape != v.shape or d.dtype != torch.float32:
            raise ValueError("weight_norm_bwd: dw must match v (fp32)")
    dvs = [torch.empty_like(v) for v in vs]
    dgs = [torch.empty_like(g) for g in gs]
    _lib.check(_lib.lib().vo_weight_norm_bwd(len(vs), _ptr_table(vs), _ptr_table(gs), _ptr_table(dws),
                                              _ptr_table(dvs), _ptr_table(dgs), rows, lens, _stream(vs[0])),
               "vo_weight_norm_bwd")
    return dvs, dgs


def wav_cl8_bwd(g):
    """Adjoint of ``wav_cl8``: g (B, T, 8) -> (B, T) fp32 (channel 0)."""
    _contig(g, "g")
    if g.shape[-1] != 8:
        raise ValueError("wav_cl8_bwd: g must end in 8 channels")
    gw = torch.empty(g.shape[:-1], dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().vo_wav_cl8_bwd(_ptr(g), vo_dtype(g), gw.numel(), _ptr(gw), _stream(g)), "vo_wav_cl8_bwd")
    return gw


def avgpool_wav_bwd(g, T):
    """Adjoint of ``avgpool_wav``: g (B, T // 2 + 1) fp32 -> (B, T) fp32."""
    _contig(g, "g")
    B = g.shape[0]
    if g.shape[1] != T // 2 + 1 or g.dtype != torch.float32:
        raise ValueError("avgpool_wav_bwd: g must be (B, T // 2 + 1) fp32")
    gx = torch.empty((B, T), dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().vo_avgpool_wav_bwd(_ptr(g), B, T, _ptr(gx), _stream(g)), "vo_avgpool_wav_bwd")
    return gx


GAN_L1, GAN_ONE_MINUS_SQ, GAN_SQ = 0, 1, 2


def _rows_view(t):
    """(..., width) view with unit column stride -> (rows, width, ld) for the reductions."""
    if t.stride(-1) != 1:
        raise ValueError("gan_reduce: last dim must be contiguous")
    width = t.shape[-1]
    lead = t.reshape(-1, width) if t.dim() != 2 else t
    if lead.dim() != 2 or (lead.shape[0] > 1 and lead.stride(0) < width):
        raise ValueError("gan_reduce: view not expressible as rows x width")
    return lead, lead.shape[0], width, lead.stride(0) if lead.shape[0] > 1 else width


def gan_reduce(kind, a, b=None, out=None):
    """sum over a of |a - b| (GAN_L1), (1 - a)^2 or a^2 -> fp32 scalar tensor (accumulated into out)."""
    la, rows, width, lda = _rows_view(a)
    ldb = 0
    if b is not None:
        lb, rb, wb, ldb = _rows_view(b)
        if (rb, wb) != (rows, width) or b.dtype != a.dtype:
            raise ValueError("gan_reduce: a / b mismatch")
        b = lb
    if out is None:
        out = torch.zeros((), dtype=torch.float32, device=a.device)
    ws = torch.empty(512, dtype=torch.float32, device=a.device)  # block partials (deterministic sum)
    _lib.check(_lib.lib().vo_gan_reduce(kind, _ptr(la), lda, _ptr(b), ldb, rows, width, vo_dtype(a), _ptr(out),
                                        _ptr(ws), _stream(a)), "vo_gan_reduce")
    return out


def gan_reduce_grad(kind, a, b, scale, out=None):
    """d(scale * sum)/da in a contiguous tensor shaped like a (scale: fp32 device scalar); ``out``: a
    contiguous tensor of a's dtype and size to write it into (returned reshaped like a)."""
    la, rows, width, lda = _rows_view(a)
    ldb = 0
    if b is not None:
        b, _, _, ldb = _rows_view(b)
    if out is not None:
        if not out.is_contiguous() or out.numel() != rows * width or out.dtype != a.dtype:
            raise ValueError("gan_reduce_grad: out must be contiguous, of a's dtype and size")
        ga = out
    else:
        ga = torch.empty((rows, width), dtype=a.dtype, device=a.device)
    _lib.check(_lib.lib().vo_gan_reduce_grad(kind, _ptr(la), lda, _ptr(b), ldb, rows, width, vo_dtype(a),
                                             _ptr(scale.float().contiguous()), _ptr(ga), width, _stream(a)),
               "vo_gan_reduce_grad")
    return ga.reshape(a.shape)


def _gan_terms(kinds, As, Bs, outs=None):
    arr = (_lib.GanTerm * len(kinds))()
    keep = []
    for i, (k, a, b) in enumerate(zip(kinds, As, Bs)):
        la, rows, width, lda = _rows_view(a)
        e = arr[i]
        e.kind, e.a, e.lda, e.rows, e.width = k, la.data_ptr(), lda, rows, width
        keep.append(la)
        if b is not None:
            lb, rb, wb, ldb = _rows_view(b)
            if (rb, wb) != (rows, width) or b.dtype != a.dtype:
                raise ValueError("gan_reduce_multi: a / b mismatch")
            e.b, e.ldb = lb.data_ptr(), ldb
            keep.append(lb)
        if outs is not None:
            o = outs[i]
            if not o.is_contiguous() or o.numel() != rows * width or o.dtype != a.dtype:
                raise ValueError("gan_reduce_grad_multi: out must be contiguous, of a's dtype and size")
            e.ga, e.ldg = o.data_ptr(), width
    if any(a.dtype != As[0].dtype for a in As):
        raise ValueError("gan_reduce_multi: one dtype for all terms")
    return arr, keep


def gan_reduce_multi(kinds, As, Bs, scale=None):
    """[gan_reduce(kinds[i], As[i], Bs[i])] * scale as one (n,) fp32 vector in one launch pair
    (vo_gan_reduce_multi; gan_reduce runs the same kernel with a table of one term, so each sum is
    gan_reduce's bit for bit).  ``scale``: (n,) fp32 device vector."""
    n = len(kinds)
    arr, keep = _gan_terms(kinds, As, Bs)
    out = torch.empty(n, dtype=torch.float32, device=As[0].device)
    L = _lib.lib()
    ws = torch.empty(int(L.vo_gan_reduce_multi_workspace_size(n)) // 4, dtype=torch.float32, device=As[0].device)
    sc = scale.float().contiguous() if scale is not None else None
    _lib.check(L.vo_gan_reduce_multi(n, ctypes.cast(arr, ctypes.c_void_p), vo_dtype(As[0]), _ptr(sc), _ptr(out),
                                     _ptr(ws), _stream(As[0])), "vo_gan_reduce_multi")
    del keep
    return out


def gan_reduce_grad_multi(kinds, As, Bs, scale, outs=None):
    """[gan_reduce_grad(kinds[i], As[i], Bs[i], scale[i])] in one launch (vo_gan_reduce_grad_multi, the kernel
    gan_reduce_grad runs with a table of one term); ``outs``: contiguous tensors to write them into (default: new tensors shaped like As)."""
    if outs is None:
        outs = [torch.empty(a.shape, dtype=a.dtype, device=a.device) for a in As]
    arr, keep = _gan_terms(kinds, As, Bs, outs)
    sc = scale.float().contiguous()
    _lib.check(_lib.lib().vo_gan_reduce_grad_multi(len(kinds), ctypes.cast(arr, ctypes.c_void_p), vo_dtype(As[0]),
                                                   _ptr(sc), _stream(As[0])), "vo_gan_reduce_grad_multi")
    del keep
    return outs


# ----------------------------------------------------------------------------- training input pipeline

def glyph_batch(strips, char_widths, cell, margin, device, W_out=None):
    """Grayscale uint8 strips (list of (H, W_b)) + per-character widths (list of int arrays, or
    None for already-centred strips) -> (B, 1, H, W_out) fp32 on ``device`` (vo_glyph_batch:
    per-character centring into ``cell`` columns, white padding, ToTensor)."""
    B = len(strips)
    H = int(strips[0].shape[0])
    widths = [int(s.shape[1]) for s in strips]
    if any(int(s.shape[0]) != H for s in strips):
        raise ValueError("glyph_batch: strips must share their height")
    offs = np.zeros(B, np.int64)
    offs[1:] = np.cumsum([H * w for w in widths])[:-1]
    packed = np.concatenate([np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) for s in strips])
    if char_widths is not None:
        cw = [np.asarray(w, np.int64).reshape(-1) for w in char_widths]
        if any(int(w.max(initial=0)) > cell for w in cw):
            raise ValueError(f"glyph_batch: a character is wider than the {cell}-pixel cell")
        for w, s in zip(cw, widths):
            if int(w.sum()) > s:
                raise ValueError("glyph_batch: character widths exceed the strip")
        char_off = np.zeros(B + 1, np.int32)
        char_off[1:] = np.cumsum([len(w) for w in cw])
        starts = np.concatenate([np.concatenate([[0], np.cumsum(w)[:-1]]) if len(w) else np.zeros(0, np.int64)
                                 for w in cw]).astype(np.int32)
        lens = np.concatenate(cw).astype(np.int32)
        w_out = max(len(w) for w in cw) * cell + 2 * margin
    else:
        char_off = starts = lens = None
        w_out = max(widths) + 2 * margin
    W_out = W_out or w_out
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(a).to(dev, non_blocking=True) if a is not None else None  # noqa: E731
    px_d, off_d, w_d = t(packed), t(offs), t(np.asarray(widths, np.int32))
    co_d, cs_d, cl_d = t(char_off), t(starts), t(lens)
    out = torch.empty((B, 1, H, W_out), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().vo_glyph_batch(_ptr(px_d), _ptr(off_d), _ptr(w_d), _ptr(co_d), _ptr(cs_d), _ptr(cl_d), B,
                                         H, int(cell), int(margin), int(W_out), _ptr(out), _stream(out)),
               "vo_glyph_batch")
    return out


def glyph_stretch_table(src_w, cell):
    """The resize coefficients of ``glyph_stretch`` for glyphs ``src_w`` pixels wide and every target width in
    1 .. cell: numpy int32 (cell (cell + 1) / 2, 2 + src_w), record w (w - 1) / 2 + c = xmin, n, K[0 .. src_w) of
    output column c at width w (vo_glyph_stretch_table; host only: no GPU call)."""
    L = _lib.lib()
    nbytes = int(L.vo_glyph_stretch_table_size(int(src_w), int(cell)))
    if nbytes < 0:
        raise ValueError(f"glyph_stretch_table: src_w must be in [1, 64] and cell in [1, 256], got ({src_w}, {cell})")
    table = np.empty((nbytes // (4 * (2 + int(src_w))), 2 + int(src_w)), np.int32)
    _lib.check(L.vo_glyph_stretch_table(int(src_w), int(cell), ctypes.c_void_p(table.ctypes.data), nbytes),
               "vo_glyph_stretch_table")
    return table


def glyph_stretch(atlas, table, ids, src_lens, widths, cell, margin, W_out=None, out=None):
    """Glyphs ``atlas`` (n_glyphs, H, S) uint8 resized per character to ``widths`` (B, T) int32 pixels (None: S, the
    glyphs as they are) and centred in ``cell``-wide cells behind ``margin`` white columns -> (B, 1, H, W_out) fp32
    = pixel / 255, W_out = T cell + 2 margin unless given (wider: white).  ``ids`` (B, T) int64 (the model's texts),
    ``src_lens`` (B,) int64, ``table`` = ``glyph_stretch_table(S, cell)``; all on the GPU, and never read on the host:
    characters past src_lens, widths <= 0 and ids outside the atlas are white cells, a width above the cell is the
    cell (vo_glyph_stretch; one launch on the current stream, graph-capturable).  ``out``: written in full."""
    if atlas.dtype != torch.uint8 or atlas.dim() != 3:
        raise ValueError(f"glyph_stretch: atlas must be uint8 (n_glyphs, H, S), got {atlas.dtype} {tuple(atlas.shape)}")
    n_glyphs, H, S = atlas.shape
    cell, margin = int(cell), int(margin)
    if ids.dtype != torch.int64 or ids.dim() != 2:
        raise ValueError(f"glyph_stretch: ids must be int64 (B, T), got {ids.dtype} {tuple(ids.shape)}")
    B, T = ids.shape
    if src_lens.dtype != torch.int64 or tuple(src_lens.shape) != (B,):
        raise ValueError(f"glyph_stretch: src_lens must be int64 ({B},), got {src_lens.dtype} {tuple(src_lens.shape)}")
    if widths is not None and (widths.dtype != torch.int32 or tuple(widths.shape) != (B, T)):
        raise ValueError(f"glyph_stretch: widths must be int32 ({B}, {T}), got {widths.dtype} {tuple(widths.shape)}")
    if table.dtype != torch.int32 or table.numel() != cell * (cell + 1) // 2 * (2 + S):
        raise ValueError(f"glyph_stretch: table is not glyph_stretch_table({S}, {cell}) as an int32 tensor")
    need = T * cell + 2 * margin
    W_out = need if W_out is None else int(W_out)
    if out is None:
        out = torch.empty((B, 1, H, W_out), dtype=torch.float32, device=atlas.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 1, H, W_out):
        raise ValueError(f"glyph_stretch: out must be fp32 {(B, 1, H, W_out)}, got {out.dtype} {tuple(out.shape)}")
    if W_out < need:
        raise ValueError(f"glyph_stretch: W_out {W_out} is below T * cell + 2 * margin = {need}")
    for name, t in (("atlas", atlas), ("table", table), ("ids", ids), ("src_lens", src_lens), ("widths", widths),
                    ("out", out)):
        if t is not None:
            _contig(t, name)
            if t.device != atlas.device:
                raise ValueError(f"glyph_stretch: {name} is on {t.device}, the atlas on {atlas.device}")
    _lib.check(_lib.lib().vo_glyph_stretch(_ptr(atlas), n_glyphs, H, S, _ptr(ids), _ptr(src_lens), _ptr(widths), B, T,
                                           cell, margin, W_out, _ptr(table), _ptr(out), _stream(out)),
               "vo_glyph_stretch")
    return out


AUGMENT_OUT = ("audiotypes", "texts", "src_lens", "mels", "mel_lens", "energies", "kurtosises", "durations", "images",
               "status")


def augment_batch(corpus, plan, T_src, T_mel, H, cell, margin, W_out=None, out=None):
    """A padded training batch from a packed base corpus (``_lib.Corpus`` of device pointers; ``dataset.DeviceCorpus``
    builds and owns one) and ``plan`` (B, 5) int32 on the GPU, rows ``src, pos, m, m_mel, r`` (include/vonoma.h states
    the index maps) -> dict of ``AUGMENT_OUT``: audiotypes (B,) int64, texts (B, T_src) int64, src_lens (B,) int64,
    mels (B, T_mel, n_mels) fp32, mel_lens (B,) fp32, energies / kurtosises / durations (B, T_src) fp32 (the first two
    None when the corpus has none), images (B, 1, H, W_out) fp32 (W_out = T_src cell + 2 margin unless given; wider:
    white), status (B,) int32.  The plan is never read on the host: a row out of range or over a cap comes out empty
    with its reason in ``status`` (``_lib.AUG_*``).  vo_augment_batch: one launch on the current stream, graph-capturable.
    ``out``: such a dict, every tensor of it written in full."""
    if not (torch.is_tensor(plan) and plan.is_cuda and plan.dtype == torch.int32 and plan.dim() == 2
            and plan.shape[1] == 5):
        raise ValueError("augment_batch: plan must be an int32 (B, 5) tensor on the GPU")
    _contig(plan, "plan")
    B, T_src, T_mel, H, cell, margin = plan.shape[0], int(T_src), int(T_mel), int(H), int(cell), int(margin)
    need = T_src * cell + 2 * margin
    W_out = need if W_out is None else int(W_out)
    if W_out < need:
        raise ValueError(f"augment_batch: W_out {W_out} is below T_src * cell + 2 * margin = {need}")
    f32, i64 = torch.float32, torch.int64
    spec = {"audiotypes": ((B,), i64), "texts": ((B, T_src), i64), "src_lens": ((B,), i64),
            "mels": ((B, T_mel, int(corpus.n_mels)), f32), "mel_lens": ((B,), f32),
            "energies": ((B, T_src), f32) if corpus.ch_energy else None,
            "kurtosises": ((B, T_src), f32) if corpus.ch_kurtosis else None,
            "durations": ((B, T_src), f32), "images": ((B, 1, H, W_out), f32), "status": ((B,), torch.int32)}
    if out is None:
        out = {k: None if s is None else torch.empty(s[0], dtype=s[1], device=plan.device) for k, s in spec.items()}
    for k, s in spec.items():
        t = out.get(k)
        if s is None:
            if t is not None:
                raise ValueError(f"augment_batch: out[{k!r}] given, but the corpus was packed without it")
            continue
        if not torch.is_tensor(t) or t.dtype != s[1] or tuple(t.shape) != s[0] or t.device != plan.device:
            raise ValueError(f"augment_batch: out[{k!r}] must be {s[1]} {s[0]} on {plan.device}, got "
                             f"{(t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else t}")
        _contig(t, k)
    _lib.check(_lib.lib().vo_augment_batch(ctypes.byref(corpus), _ptr(plan), B, T_src, T_mel, H, cell, margin, W_out,
                                           *[_ptr(out[k]) for k in AUGMENT_OUT], _stream(plan)),
               "vo_augment_batch")
    return out


STATS_FEATURES = {"energy": _lib.STATS_ENERGY, "kurtosis": _lib.STATS_KURTOSIS}


def corpus_stats(corpus, plan, feature, out=None, status=None, workspace=None):
    """The reference's energy / kurtosis statistics over the variants of ``plan`` without the variants (include/vonoma.h,
    vo_corpus_stats).  ``corpus``: a ``_lib.Corpus`` of device pointers (``dataset.DeviceCorpus``
    owns one), ``plan`` (n_rows, 5) int32 on the GPU, rows ``src, pos, m, m_mel, r``, ``feature`` "energy" or "kurtosis"
    (or ``_lib.STATS_*``) -> (out, status): out (6,) float64 = kept count, mean, std, raw min, raw max, rows that kept
    a value; status (n_rows,) int32 (``_lib.AUG_BAD_ROW`` or ``_lib.STATS_CHARS_OVER`` for a row that was refused and
    contributed nothing).  The plan is never read on the host (``DeviceCorpus.stats`` checks a host plan first).  Two
    launches on the current stream, no atomics, graph-capturable.  ``out`` / ``status`` / ``workspace`` (uint8,
    ``vo_corpus_stats_workspace_size(n_rows)`` bytes or more): tensors of an earlier call, written in full."""
    if not (torch.is_tensor(plan) and plan.is_cuda and plan.dtype == torch.int32 and plan.dim() == 2
            and plan.shape[1] == 5 and plan.shape[0] >= 1):
        raise ValueError("corpus_stats: plan must be an int32 (n_rows, 5) tensor on the GPU with n_rows >= 1")
    _contig(plan, "plan")
    f = STATS_FEATURES.get(feature, feature)
    if f not in STATS_FEATURES.values():
        raise ValueError(f"corpus_stats: feature must be one of {tuple(STATS_FEATURES)}, got {feature!r}")
    if not (corpus.ch_energy if f == _lib.STATS_ENERGY else corpus.ch_kurtosis):
        raise ValueError(f"corpus_stats: the corpus was packed without {('energy', 'kurtosis')[f]}")
    n_rows = plan.shape[0]
    need = int(_lib.lib().vo_corpus_stats_workspace_size(n_rows))
    spec = {"out": ((6,), torch.float64), "status": ((n_rows,), torch.int32)}
    given = {"out": out, "status": status}
    for k, (shape, dt) in spec.items():
        t = given[k]
        if t is None:
            given[k] = torch.empty(shape, dtype=dt, device=plan.device)
        elif not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or t.device != plan.device:
            raise ValueError(f"corpus_stats: {k} must be {dt} {shape} on {plan.device}, got "
                             f"{(t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else t}")
        else:
            _contig(t, k)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=plan.device)
    elif (not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1
          or workspace.numel() < need or workspace.device != plan.device):
        raise ValueError(f"corpus_stats: workspace must be uint8 ({need},) or longer on {plan.device}")
    else:
        _contig(workspace, "workspace")
    _lib.check(_lib.lib().vo_corpus_stats(ctypes.byref(corpus), _ptr(plan), n_rows, f, _ptr(workspace),
                                          workspace.numel(), _ptr(given["out"]), _ptr(given["status"]), _stream(plan)),
               "vo_corpus_stats")
    return given["out"], given["status"]


def corpus_normalize_(values, stats):
    """``values`` (fp32, any shape, contiguous) <- (float)(((double)values - stats[1]) / stats[2]) in place, ``stats`` the
    (6,) float64 ``out`` of ``corpus_stats`` on the same device, read there: stream-ordered behind that call without a
    host round trip (vo_corpus_normalize; one launch on the current stream, graph-capturable).  numpy's float64
    ``(x - mean) / std`` followed by ``.astype(float32)``, bit for bit."""
    if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.numel() >= 1):
        raise ValueError("corpus_normalize_: values must be a non-empty fp32 tensor on the GPU")
    if not (torch.is_tensor(stats) and stats.dtype == torch.float64 and tuple(stats.shape) == (6,)
            and stats.device == values.device):
        raise ValueError(f"corpus_normalize_: stats must be float64 (6,) on {values.device} (corpus_stats's out)")
    _contig(values, "values")
    _contig(stats, "stats")
    _lib.check(_lib.lib().vo_corpus_normalize(_ptr(values), values.numel(), _ptr(stats), _stream(values)),
               "vo_corpus_normalize")
    return values


SEGMENT_OUT = ("y", "x", "frames", "status")


def _segment_sizes(who, B, fps):
    B, fps = int(B), int(fps)
    if not 1 <= B <= 65535:
        raise ValueError(f"{who}: B must be in [1, 65535], got {B}")
    if fps < 1:
        raise ValueError(f"{who}: fps must be >= 1, got {fps}")
    return B, fps


def segment_batch(corpus, waves, plan, fps, hop, mel_pad=0.0, out=None):
    """Aligned (mel, audio) training segments of the vocoder from a packed corpus (``_lib.Corpus``), the waveforms
    beside it (``_lib.WaveCorpus``; ``dataset.DeviceCorpus.attach_waves`` builds and owns one) and ``plan`` (B, 2)
    int32 on the GPU, rows ``src, start`` with start in frames (include/vonoma.h states the rule) -> dict of
    ``SEGMENT_OUT``: y (B, fps * hop) fp32, x (B, fps, n_mels) fp32 channels-last, frames (B,) int32, status (B,)
    int32.  Past an utterance's end y is 0.0 and x is ``mel_pad``.  The plan is never read on the host: a row out of
    range comes out as padding with ``_lib.SEG_BAD_ROW`` in ``status``.  vo_segment_batch: one launch on the current
    stream, graph-capturable.  ``out``: such a dict, every tensor of it written in full."""
    if not (torch.is_tensor(plan) and plan.is_cuda and plan.dtype == torch.int32 and plan.dim() == 2
            and plan.shape[1] == 2):
        raise ValueError("segment_batch: plan must be an int32 (B, 2) tensor on the GPU")
    _contig(plan, "plan")
    B, fps = _segment_sizes("segment_batch", plan.shape[0], fps)
    hop, n_mels = int(hop), int(corpus.n_mels)
    if hop < 1:
        raise ValueError(f"segment_batch: hop must be >= 1, got {hop}")
    if fps * hop >= 2 ** 31 or fps * n_mels >= 2 ** 31:
        raise ValueError(f"segment_batch: a row of fps * hop = {fps * hop} samples or fps * n_mels = {fps * n_mels} "
                         "values is at or above 2^31")
    if int(waves.U) != int(corpus.U):
        raise ValueError(f"segment_batch: the wave corpus has {int(waves.U)} utterances, the corpus {int(corpus.U)}")
    spec = {"y": ((B, fps * hop), torch.float32), "x": ((B, fps, n_mels), torch.float32),
            "frames": ((B,), torch.int32), "status": ((B,), torch.int32)}
    if out is None:
        out = {k: torch.empty(s[0], dtype=s[1], device=plan.device) for k, s in spec.items()}
    for k, s in spec.items():
        t = out.get(k)
        if not torch.is_tensor(t) or t.dtype != s[1] or tuple(t.shape) != s[0] or t.device != plan.device:
            raise ValueError(f"segment_batch: out[{k!r}] must be {s[1]} {s[0]} on {plan.device}, got "
                             f"{(t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else t}")
        _contig(t, k)
    _lib.check(_lib.lib().vo_segment_batch(ctypes.byref(corpus), ctypes.byref(waves), _ptr(plan), B, fps, hop,
                                           float(mel_pad), *[_ptr(out[k]) for k in SEGMENT_OUT], _stream(plan)),
               "vo_segment_batch")
    return out


def segment_plan(corpus, order, counter, seed, B, fps, plan=None):
    """The next ``B`` rows of the vocoder's segment draw -> plan (B, 2) int32, rows ``src, start`` (vo_segment_plan,
    include/vonoma.h): row b from k = counter + b, src = order[k mod len(order)], start uniform in [0, max(F - fps, 0)]
    from Philox4x32-10 of k under ``seed``; then ``counter`` += B on the device.  ``order`` (n_order,) int32 and
    ``counter`` (1,) int64 live on the GPU and are never read on the host: one launch on the current stream,
    graph-capturable, and a replay draws the following rows.  ``hifigan.data.segment_plan_host`` is the same rule in
    numpy.  ``plan``: the tensor of an earlier call, written in full."""
    if not (torch.is_tensor(order) and order.is_cuda and order.dtype == torch.int32 and order.dim() == 1
            and order.shape[0] >= 1):
        raise ValueError("segment_plan: order must be a non-empty int32 (n_order,) tensor on the GPU")
    if not (torch.is_tensor(counter) and counter.dtype == torch.int64 and counter.numel() == 1
            and counter.device == order.device):
        raise ValueError(f"segment_plan: counter must be one int64 on {order.device}")
    _contig(order, "order")
    B, fps = _segment_sizes("segment_plan", B, fps)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"segment_plan: seed must be in [0, 2^64), got {seed}")
    if plan is None:
        plan = torch.empty((B, 2), dtype=torch.int32, device=order.device)
    elif (not torch.is_tensor(plan) or plan.dtype != torch.int32 or tuple(plan.shape) != (B, 2)
          or plan.device != order.device):
        raise ValueError(f"segment_plan: plan must be int32 ({B}, 2) on {order.device}")
    else:
        _contig(plan, "plan")
    _lib.check(_lib.lib().vo_segment_plan(ctypes.byref(corpus), _ptr(order), order.shape[0], _ptr(counter), seed, B,
                                          fps, _ptr(plan), _stream(order)), "vo_segment_plan")
    return plan


# ----------------------------------------------------------------------------- sample-rate conversion

RESAMPLE_TILE = 256  # the outputs one workgroup of resample_kernel writes (RS_TILE, csrc/resample.hip)
_RESAMPLE_TABLES = {}


def resample_geometry(sr_in, sr_out):
    """(O, M, W) of a conversion from ``sr_in`` to ``sr_out`` (vo_resample_geometry, host only): the reduced rates
    and the filter's half width in input samples; T = 2 W + 1 taps.  ValueError, with the library's message naming
    the reduced pair and the limits, for equal rates, a rate < 1, O or M above 1024 and O / M above 8."""
    L = _lib.lib()
    O, M, W = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    if L.vo_resample_geometry(int(sr_in), int(sr_out), ctypes.byref(O), ctypes.byref(M), ctypes.byref(W)) != 0:
        raise ValueError(L.vo_last_error().decode(errors="replace"))
    return O.value, M.value, W.value


def resample_len(n, O, M):
    """ceil(n M / O): the samples ``n`` input samples become (vo_resample_len, host only)."""
    return int(_lib.lib().vo_resample_len(int(n), int(O), int(M)))


def resample_table(O, M, device=None):
    """The (M, 2 W + 1) fp32 coefficients of the reduced pair (vo_resample_table: double, rounded once).  With
    ``device`` the copy on that device, built once and cached; without, a new host tensor."""
    if device is not None:
        key = (O, M, str(torch.device(device)))
        if key not in _RESAMPLE_TABLES:
            _RESAMPLE_TABLES[key] = resample_table(O, M).to(device)
        return _RESAMPLE_TABLES[key]
    W = resample_geometry(O, M)[2]  # refuses what the library does not run; (O, M) must already be reduced
    t = torch.empty((M, 2 * W + 1), dtype=torch.float32)
    _lib.check(_lib.lib().vo_resample_table(O, M, ctypes.c_void_p(t.data_ptr())), "vo_resample_table")
    return t


def _resample_rows(v, B, hi, ref, name):
    """``lens`` / ``skip`` of ``resample`` -> contiguous int32 (B,) on ``ref``'s device.  A device tensor (int32 /
    int64) is converted on the device and never read on the host (the kernel clamps it); a host sequence is
    validated here: B integers in [0, hi]."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype not in (torch.int32, torch.int64) or v.shape != (B,):
            raise ValueError(f"resample: {name} must be an int32 / int64 tensor of shape ({B},), got {v.dtype} "
                             f"{tuple(v.shape)}")
        if v.device != ref.device:
            raise ValueError(f"resample: {name} is on {v.device}, the waveform on {ref.device}")
        return v.to(torch.int32).contiguous()
    host = [int(a) for a in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if len(host) != B or any(a < 0 or a > hi for a in host):
        raise ValueError(f"resample: {name} must be {B} sample counts in [0, {hi}], got {host}")
    return torch.tensor(host, dtype=torch.int32).to(ref.device)


def resample(x, sr_in, sr_out, lens=None, skip=None, max_wav_value=None, pcm_scale=None, out=None,
             out_capacity=None):
    """Sample-rate conversion of a ragged batch in one launch (vo_resample; include/vonoma.h states the rule: a
    Kaiser-windowed sinc of 64 zero crossings): x (B, N) fp32, or int16 read as s / ``max_wav_value`` (32768.0 by
    default), at ``sr_in`` -> (y, out_lens) at ``sr_out``.  Row b holds ``lens[b]`` samples (None: N) and loses its
    first ``skip[b]`` output samples (None: 0; clamped to the row's length).  y is (B, N_out) with N_out =
    ``out_capacity``, or ``out``'s, or resample_len(N): fp32, or int16 with ``pcm_scale`` (the store of
    ``Generator.run(pcm_scale=...)``); row b holds out_lens[b] = clamp(ceil(lens[b] M / O) - skip[b], 0, N_out)
    samples, then zeros.  out_lens is int32 (B,) on the device.  ``lens`` and ``skip``: int32 / int64 device
    tensors, never read on the host (the call is graph-capturable and a replay follows them, and x, changed in
    place), or host sequences, which are validated.  Equal rates are a ValueError: there is nothing to launch."""
    if not (torch.is_tensor(x) and x.dim() == 2 and x.dtype in (torch.float32, torch.int16)):
        raise ValueError("resample: x must be an fp32 or int16 (B, N) tensor, got "
                         f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__}")
    st = _stream(x)
    _contig(x, "x")
    O, M, _ = resample_geometry(sr_in, sr_out)
    B, N = x.shape
    if not 1 <= B <= 65535 or N < 1:
        raise ValueError(f"resample: x is {(B, N)}: B must be in [1, 65535] and N >= 1")
    is16 = x.dtype == torch.int16
    if max_wav_value is not None and not is16:
        raise ValueError("resample: max_wav_value belongs to int16 input, x is fp32")
    mwv = 32768.0 if max_wav_value is None else float(max_wav_value)
    if not (0.0 < mwv < float("inf")):
        raise ValueError(f"resample: max_wav_value must be finite and positive, got {max_wav_value}")
    if pcm_scale is not None and not (0.0 < float(pcm_scale) < float("inf")):
        raise ValueError(f"resample: pcm_scale must be finite and positive, got {pcm_scale}")
    y_dtype = torch.float32 if pcm_scale is None else torch.int16
    if out_capacity is not None:
        N_out = int(out_capacity)
    elif out is not None:
        N_out = out.shape[1] if out.dim() == 2 else -1
    else:
        N_out = resample_len(N, O, M)
    if not 1 <= N_out < 2 ** 31 - RESAMPLE_TILE:
        raise ValueError(f"resample: the output capacity must be in [1, 2^31 - {RESAMPLE_TILE}), got {N_out}")
    if out is None:
        out = torch.empty((B, N_out), dtype=y_dtype, device=x.device)
    elif tuple(out.shape) != (B, N_out) or out.dtype != y_dtype or out.device != x.device:
        raise ValueError(f"resample: out must be {y_dtype} {(B, N_out)} on {x.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    _contig(out, "out")
    lens32 = None if lens is None else _resample_rows(lens, B, N, x, "lens")
    skip32 = None if skip is None else _resample_rows(skip, B, 2 ** 31 - 1, x, "skip")
    table = resample_table(O, M, x.device)
    out_lens = torch.empty(B, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().vo_resample(_ptr(x), int(is16), mwv, B, N, _ptr(lens32), _ptr(skip32), _ptr(table), O, M,
                                      _ptr(out), int(pcm_scale is not None), float(pcm_scale or 0.0), N_out,
                                      _ptr(out_lens), st), "vo_resample")
    return out, out_lens


# ----------------------------------------------------------------------------- offline feature extraction

def spec_features(wav, window, fb, n_fft=1024, hop=256, log_floor=1e-5):
    """torchaudio-framed log-mel (B, n_mels, F), frame energy (B, F) and per-frame power
    statistics (B, F, 2) of wav (B, N) (vo_stft_mel_ex, clipped input, center=True)."""
    _contig(wav, "wav")
    B, N = wav.shape
    F = 1 + N // hop
    mel = torch.empty((B, fb.shape[1], F), dtype=torch.float32, device=wav.device)
    energy = torch.empty((B, F), dtype=torch.float32, device=wav.device)
    fstats = torch.empty((B, F, 2), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().vo_stft_mel_ex(_ptr(wav), B, N, _ptr(window), _ptr(fb), n_fft, hop, fb.shape[1],
                                         n_fft // 2, 0.0, 1, float(log_floor), _ptr(mel), _ptr(energy),
                                         _ptr(fstats), _stream(wav)), "vo_stft_mel_ex")
    return mel, energy, fstats


def char_features(energy, fstats, durations, n_bins, flat=False):
    """energy (B, F), fstats (B, F, 2), durations: list of B int arrays -> (energy_char, kurtosis_char)
    lists (per-character mean energy, spectral kurtosis) via vo_char_features.  ``flat``: the utterances'
    characters concatenated instead, (energy_char (n,), kurtosis_char (n,), off) with utterance b's at
    [off[b], off[b + 1]) (off: host int32 (B + 1,)) -- one buffer per output kind, for one copy to the host."""
    B, F = energy.shape
    dur = np.concatenate([np.asarray(d, np.int32).reshape(-1) for d in durations])
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in durations])
    dev = energy.device
    dur_d, off_d = torch.from_numpy(dur).to(dev), torch.from_numpy(off).to(dev)
    e = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
    k = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().vo_char_features(_ptr(energy.contiguous()), _ptr(fstats.contiguous()), F, _ptr(dur_d),
                                           _ptr(off_d), B, int(n_bins), _ptr(e), _ptr(k), _stream(energy)),
               "vo_char_features")
    if flat:
        return e, k, off
    return [e[off[i]:off[i + 1]] for i in range(B)], [k[off[i]:off[i + 1]] for i in range(B)]


# ----------------------------------------------------------------------------- training backward

def conv1d_wgrad(a, b, K, S=1, dil=1, pad=0, pre_a=None, pre_b=None, transposed=False, groups=1, with_bias=False,
                 split=False):
    """Weight gradient on MFMA (vo_conv1d_wgrad_bias).  Conv1d: a = dY (B, T_out, Co), b = x (B, T_in, Ci)
    -> dW (Co, Ci / groups, K).  ConvTranspose1d (transposed=True): a = x (B, T_in, Ci), b = dY
    (B, T_up, Co) -> dW (Ci, Co, K).  pre_a / pre_b: leaky-ReLU slope applied to that operand
    (None = identity).  with_bias (conv form): also the bias gradient, column sums of a, from the
    same launch (vo_conv1d_wgrad_bias) -> (dW, db).  split (fp32 operands, stride 1, ungrouped): contract
    them as split-bf16 (VO_F32X3, see F32X3)."""
    _contig(a, "a")
    _contig(b, "b")
    if a.dtype != b.dtype:
        raise TypeError("conv1d_wgrad: operand dtypes differ")
    B, T_A, M = a.shape
    _, T_B, N = b.shape
    if M % groups or N % groups:
        raise ValueError(f"conv1d_wgrad: channels {M} / {N} not divisible by groups {groups}")
    if with_bias and (pre_a is not None or transposed):
        raise ValueError("conv1d_wgrad: the fused bias gradient needs the conv form with a = dY as stored")
    mg, ng = M // groups, N // groups
    L = _lib.lib()
    w = torch.empty((M, ng, K), dtype=torch.float32, device=a.device)  # written in weight order
    db = torch.empty(M, dtype=torch.float32, device=a.device) if with_bias else None
    ws = torch.empty(int(L.vo_conv1d_wgrad_workspace_size(B, T_A, mg, ng, K, groups)) // 4, dtype=torch.float32,
                     device=a.device)  # row-split partials, added in a fixed order (deterministic)
    slope = pre_a if pre_a is not None else (pre_b if pre_b is not None else 0.0)
    if pre_a is not None and pre_b is not None and pre_a != pre_b:
        raise ValueError("conv1d_wgrad: one slope for both operands")
    dt = vo_dtype(a)
    if split:
        if a.dtype != torch.float32 or S != 1 or groups != 1 or transposed:
            raise ValueError("conv1d_wgrad: split needs fp32 operands, stride 1, ungrouped, conv form")
        dt = VO_F32X3
    _lib.check(L.vo_conv1d_wgrad_bias(_ptr(a), M, T_A, _ptr(b), N, T_B, B, mg, ng, K, S, dil, pad, groups,
                                      int(pre_a is not None), int(pre_b is not None), float(slope), dt,
                                      _ptr(w), _ptr(db), _ptr(ws), _stream(a)), "vo_conv1d_wgrad_bias")
    return (w, db) if with_bias else w


WGRAD_LAUNCH_FIELDS = ("ROUTE", "TM", "KG", "SW", "ntg", "gpt", "splits", "rows_per_split", "direct", "reduce_W",
                       "compute_dtype", "bias")
WGRAD_PER_TAP, WGRAD_MULTI_TAP, WGRAD_K1 = 1, 2, 3  # ROUTE


def conv1d_wgrad_plan(B, T_A, T_B, M, N, K, S=1, dil=1, pad=0, groups=1, pre_a=False, pre_b=False, dtype=VO_BF16,
                      with_bias=False):
    """The launch record ``vo_conv1d_wgrad_bias`` with these sizes (M, N per group) would leave, a dict over
    WGRAD_LAUNCH_FIELDS, without launching anything (vo_conv1d_wgrad_plan: the routing the launch itself runs,
    vo_tune knobs included).  Host only."""
    rec = (ctypes.c_int32 * len(WGRAD_LAUNCH_FIELDS))()
    _lib.check(_lib.lib().vo_conv1d_wgrad_plan(B, T_A, T_B, M, N, K, S, dil, pad, groups, int(bool(pre_a)),
                                               int(bool(pre_b)), dtype, int(bool(with_bias)), rec,
                                               len(WGRAD_LAUNCH_FIELDS)), "vo_conv1d_wgrad_plan")
    return dict(zip(WGRAD_LAUNCH_FIELDS, (int(v) for v in rec)))


def conv1d_wgrad_last_launch():
    """What the calling thread's last weight-gradient call launched, as a dict over WGRAD_LAUNCH_FIELDS
    (vo_conv1d_wgrad_last_launch in include/vonoma.h); all zeros when the call was rejected."""
    rec = (ctypes.c_int32 * len(WGRAD_LAUNCH_FIELDS))()
    n = _lib.lib().vo_conv1d_wgrad_last_launch(rec, len(WGRAD_LAUNCH_FIELDS))
    if n != len(WGRAD_LAUNCH_FIELDS):
        raise RuntimeError(f"vo_conv1d_wgrad_last_launch returned {n} fields, expected {len(WGRAD_LAUNCH_FIELDS)}")
    return dict(zip(WGRAD_LAUNCH_FIELDS, (int(v) for v in rec)))


def lrelu_mask(g, ref, slope, out=None, add=None, summand=None):
    """g * (ref > 0 ? 1 : slope) (leaky-ReLU / ReLU backward); g, ref (..., C) with row-contiguous
    last dims (ref may be a channel slice of a wider tensor).  out=g computes in place.  ``add``
    (g's shape and dtype): that rounded result plus ``add`` in the same pass (vo_lrelu_mask_add).
    ``summand`` (g's shape and dtype): the mask of round(g + summand) (vo_lrelu_mask_sum)."""
    if g.shape != ref.shape:
        raise ValueError("lrelu_mask: g and ref shapes differ")
    if add is not None and summand is not None:
        raise ValueError("lrelu_mask: add or summand, not both")
    if summand is not None:
        if summand.shape != g.shape or summand.dtype != g.dtype:
            raise ValueError("lrelu_mask: summand must match g")
        C = g.shape[-1]
        g, ref, summand = g.contiguous(), ref.contiguous(), summand.contiguous()
        out = torch.empty_like(g) if out is None else _contig(out, "out")
        _lib.check(_lib.lib().vo_lrelu_mask_sum(_ptr(g), C, vo_dtype(g), _ptr(ref), C, vo_dtype(ref), _ptr(summand),
                                                C, g.numel() // C, C, float(slope), _ptr(out), C, _stream(g)),
                   "vo_lrelu_mask_sum")
        return out
    if add is not None:
        if add.shape != g.shape or add.dtype != g.dtype:
            raise ValueError("lrelu_mask: add must match g")
        C = g.shape[-1]
        g, ref, add = g.contiguous(), ref.contiguous(), add.contiguous()
        out = torch.empty_like(g) if out is None else _contig(out, "out")
        _lib.check(_lib.lib().vo_lrelu_mask_add(_ptr(g), C, vo_dtype(g), _ptr(ref), C, vo_dtype(ref), _ptr(add), C,
                                                g.numel() // C, C, float(slope), _ptr(out), C, _stream(g)),
                   "vo_lrelu_mask_add")
        return out
    C = g.shape[-1]

    def row_strided(t):  # (..., C) rows at a common stride (a channel slice of a wider tensor is fine)
        return t.dim() >= 2 and t.stride(-1) == 1 and all(
            t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2))
    if not row_strided(g):
        g, out = g.contiguous(), None
    if not row_strided(ref):
        ref = ref.contiguous()
    if out is not None and not row_strided(out):
        raise ValueError("lrelu_mask: out must be row-strided (..., C)")
    out = torch.empty(g.shape, dtype=g.dtype, device=g.device) if out is None else out
    rows = g.numel() // C
    ld = lambda t: t.stride(-2)  # noqa: E731
    _lib.check(_lib.lib().vo_lrelu_mask(_ptr(g), ld(g), vo_dtype(g), _ptr(ref), ld(ref), vo_dtype(ref), rows, C,
                                        float(slope), _ptr(out), ld(out), _stream(g)), "vo_lrelu_mask")
    return out


def colsum(x):
    """(..., C) -> (C,) fp32 column sums (bias gradient)."""
    _contig(x, "x")
    C = x.shape[-1]
    if C % 8:
        x = torch.nn.functional.pad(x, (0, 8 - C % 8)).contiguous()
        return colsum(x)[:C]
    rows = x.numel() // C
    L = _lib.lib()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.vo_colsum_workspace_size(rows, C)) // 4, dtype=torch.float32, device=x.device)
    _lib.check(L.vo_colsum(_ptr(x), rows, C, C, vo_dtype(x), _ptr(out), _ptr(ws), _stream(x)), "vo_colsum")
    return out
