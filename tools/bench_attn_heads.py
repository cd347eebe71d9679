#!/usr/bin/env python
"""Attention at head counts 2, 4 and 8 (d_k = 128, 64, 32 at hidden 256) against the reference's formulation.

Two shapes: the decoder's (B = 32, L = 512, bf16) and the encoder's (B = 32, L = 12, fp32), ragged lengths from a
fixed seed.  Per head count, timed per call with device events over blocks of whole calls, after a warm-up, every
variant of a shape alternating block by block (att_xcd at its default):

    hip_fwd    ops.attention(qkv, lens, H, with_lse=True)
    hip_bwd    ops.attention_bwd(qkv, out, dout, lens, H, lse)
    torch_fwd  bmm -> masked_fill -> softmax -> bmm on q / k / v already split into (B H, L, d_k) (the head split and
               merge copies of the reference are left out of the timed region: a floor that favours torch)
    torch_fb   that chain and its autograd backward

H = 2, 4 and 8 do the same matmul FLOPs; the softmax work per FLOP doubles each time d_k halves.  Reported: medians,
each block, the ratio to H = 2, and whether the HIP path beats the torch chain by more than the run-to-run spread
(the larger of the two variants' max - min over their blocks).  Prints one JSON line; exit status 1 if a HIP path at
H = 4 or 8 does not beat the chain.

    python tools/bench_attn_heads.py [--blocks 5] [--window 0.2]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"decoder": dict(B=32, L=512, D=256, dtype=torch.bfloat16, min_len=128),
          "encoder": dict(B=32, L=12, D=256, dtype=torch.float32, min_len=4)}
HEADS = (2, 4, 8)


def variants(s, H, gen):
    from visual_onoma_to_wave_amd import ops
    B, L, D, dt = s["B"], s["L"], s["D"], s["dtype"]
    dk = D // H
    qkv = torch.randn(B, L, 3 * D, generator=gen, device="cuda").to(dt)
    dout = torch.randn(B, L, D, generator=gen, device="cuda").to(dt)
    lens = torch.randint(s["min_len"], L + 1, (B,), generator=gen, device="cuda").to(torch.int32)
    lens[0] = L
    out, lse = ops.attention(qkv, lens, H, with_lse=True)
    # the reference's operands: heads batched head-major, (H B, L, d_k)
    q, k, v = (t.reshape(B, L, H, dk).permute(2, 0, 1, 3).reshape(H * B, L, dk).contiguous().requires_grad_()
               for t in qkv.split(D, dim=-1))
    mask = (torch.arange(L, device="cuda")[None, :] >= lens[:, None])[:, None, :].expand(-1, L, -1).repeat(H, 1, 1)
    go = dout.reshape(B, L, H, dk).permute(2, 0, 1, 3).reshape(H * B, L, dk).contiguous()
    scale = 1.0 / dk ** 0.5

    def chain():
        a = torch.softmax((torch.bmm(q, k.transpose(1, 2)) * scale).masked_fill(mask, -float("inf")), dim=2)
        return torch.bmm(a, v)

    def torch_fwd():
        with torch.no_grad():
            chain()

    def torch_fb():
        q.grad = k.grad = v.grad = None
        chain().backward(go)

    with torch.no_grad():
        ref = chain().reshape(H, B, L, dk).permute(1, 2, 0, 3).reshape(B, L, D)
    err = float((out.float() - ref.float()).norm() / ref.float().norm())
    assert err < (2e-2 if dt == torch.bfloat16 else 1e-4), err  # both paths compute the same thing
    return {"hip_fwd": lambda: ops.attention(qkv, lens, H, with_lse=True),
            "hip_bwd": lambda: ops.attention_bwd(qkv, out, dout, lens, H, lse),
            "torch_fwd": torch_fwd, "torch_fb": torch_fb}


def block(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per variant (alternating)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed block, at least")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_heads: no GPU")
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    res, ok = {}, True
    for name, s in SHAPES.items():
        fns = {(H, k): f for H in HEADS for k, f in variants(s, H, gen).items()}
        runs = {}
        for key, fn in fns.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            runs[key] = max(3, int(a.window * 1000.0 / block(fn, 5)) + 1)
        times = {key: [] for key in fns}
        for _ in range(a.blocks):
            for key, fn in fns.items():
                times[key].append(block(fn, runs[key]))
        med = {key: statistics.median(t) for key, t in times.items()}
        spread = {key: max(t) - min(t) for key, t in times.items()}
        r = dict(shape=[s["B"], s["L"], s["D"]], dtype=str(s["dtype"]).replace("torch.", ""), heads={})
        for H in HEADS:
            hf, hb, tf, tb = (H, "hip_fwd"), (H, "hip_bwd"), (H, "torch_fwd"), (H, "torch_fb")
            fwd_ok = med[tf] - med[hf] > max(spread[tf], spread[hf])
            fb_ok = med[tb] - (med[hf] + med[hb]) > max(spread[tb], spread[hf] + spread[hb])
            if H != 2:
                ok = ok and fwd_ok and fb_ok
            r["heads"][H] = dict(
                d_k=s["D"] // H,
                us={k: round(1000 * med[H, k], 2) for k in ("hip_fwd", "hip_bwd", "torch_fwd", "torch_fb")},
                blocks_us={k: [round(1000 * t, 2) for t in times[H, k]]
                           for k in ("hip_fwd", "hip_bwd", "torch_fwd", "torch_fb")},
                fwd_over_h2=round(med[hf] / med[2, "hip_fwd"], 3), bwd_over_h2=round(med[hb] / med[2, "hip_bwd"], 3),
                torch_fwd_over_hip=round(med[tf] / med[hf], 2),
                torch_fb_over_hip=round(med[tb] / (med[hf] + med[hb]), 2),
                hip_fwd_beats_torch=bool(fwd_ok), hip_fwd_bwd_beats_torch=bool(fb_ok))
        res[name] = r
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
