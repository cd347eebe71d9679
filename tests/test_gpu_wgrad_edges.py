"""Every weight-gradient kernel of csrc/wgrad.hip at its edges, per element against float64 (tests/wgrad_check.py:
the derived bar, NaN sentinel rows and channels around both operands, guard bands around dW, db and the
workspace, a NaN-filled workspace, two runs that must agree bit for bit).

Each case calls vo_conv1d_wgrad_bias through the ctypes binding with the raw pointers of the guarded views
(leading dimensions wider than groups x M / groups x N, which ops.conv1d_wgrad cannot pass) and asserts the
launch record (ops.conv1d_wgrad_last_launch) right after the call against the record the case declares: a
change to the routing rules, to wgrad_mt_plan or to k1_plan that moves a case onto another kernel fails here,
and already in the CPU suite (tests/test_wgrad_check.py checks every declared record against
vo_conv1d_wgrad_plan, and REQUIRED against what the cases reach).

Sizes are the smallest at which each path exists: B = 3 unless the plan needs more, the reduction length
R = B T_A never above 1200 (wgrad_check: a dropped row stays >= 5.8 bars away).
"""

import pytest
import torch

import wgrad_check as WC
from wgrad_check import case

CASES = [
    # per-tap kernel, bf16: direct and partials + reduce at one split, splits cut inside an utterance with a one-row
    # last chunk, 40 x 72 tiles, pre_b, bias on and off, pad > T
    case(3, 40, 40, 72, 3, pad=1, bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 40, 40, 72, 3, pad=1, knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 40, 64, 64, 3, pad=1, bias=True, knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 107, 64, 64, 3, pad=1, pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 107, 40, 72, 5, pad=2, bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 27, 64, 64, 7, dil=3, pad=20, pre_b=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 27, 40, 72, 7, dil=3, pad=20, bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    # per-tap kernel, f32: direct and partials + reduce at one split, splits cut inside an utterance with a one-row
    # last chunk, 40 x 72 tiles, pre_b, bias on and off, pad > T
    case(3, 40, 40, 72, 3, pad=1, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 40, 40, 72, 3, pad=1, dt="f32", knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 40, 64, 64, 3, pad=1, dt="f32", bias=True, knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 107, 64, 64, 3, pad=1, dt="f32", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 107, 40, 72, 5, pad=2, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 27, 64, 64, 7, dil=3, pad=20, dt="f32", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 27, 40, 72, 7, dil=3, pad=20, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    # per-tap kernel, x3: direct and partials + reduce at one split, splits cut inside an utterance with a one-row
    # last chunk, 40 x 72 tiles, pre_b, bias on and off, pad > T
    case(3, 40, 40, 72, 3, pad=1, dt="x3", bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 40, 40, 72, 3, pad=1, dt="x3", knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 40, 64, 64, 3, pad=1, dt="x3", bias=True, knobs={"wgrad_cfg": 13}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 0, 1)),
    case(3, 107, 64, 64, 3, pad=1, dt="x3", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 107, 40, 72, 5, pad=2, dt="x3", bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 27, 64, 64, 7, dil=3, pad=20, dt="x3", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 27, 40, 72, 7, dil=3, pad=20, dt="x3", bias=True, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    # per-tap kernel, bf16: strides, groups packed per tile (gpt) or not, the transposed form
    case(3, 100, 32, 64, 5, S=2, pad=2, pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=3, pad=2, bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=4, pad=2, pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=8, pad=2, pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 16, 8, 5, S=2, pad=2, groups=16, bias=True, pre_b=True, rec=(1, 64, 0, 0, 0, 4, 3, 128, 0, 1)),
    case(3, 100, 32, 32, 3, pad=1, groups=4, bias=True, rec=(1, 64, 0, 0, 0, 2, 3, 128, 0, 1)),
    case(3, 100, 64, 32, 3, pad=1, groups=2, bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 40, 16, 8, 3, pad=1, groups=16, bias=True, knobs={"wgrad_cfg": 12}, rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 20, 64, 32, 16, S=8, pad=4, pre_a=True, transposed=True, rec=(1, 64, 0, 0, 0, 1, 1, 64, 1, 0)),
    case(3, 107, 64, 32, 16, S=8, pad=4, pre_a=True, transposed=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    # per-tap kernel, f32: strides, groups packed per tile (gpt) or not, the transposed form
    case(3, 100, 32, 64, 5, S=2, pad=2, dt="f32", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=3, pad=2, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=4, pad=2, dt="f32", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 32, 64, 5, S=8, pad=2, dt="f32", pre_b=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 100, 16, 8, 5, S=2, pad=2, groups=16, dt="f32", bias=True, pre_b=True,
         rec=(1, 64, 0, 0, 0, 4, 3, 128, 0, 1)),
    case(3, 100, 32, 32, 3, pad=1, groups=4, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 2, 3, 128, 0, 1)),
    case(3, 100, 64, 32, 3, pad=1, groups=2, dt="f32", bias=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    case(3, 40, 16, 8, 3, pad=1, groups=16, dt="f32", bias=True, knobs={"wgrad_cfg": 12},
         rec=(1, 64, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 20, 64, 32, 16, S=8, pad=4, dt="f32", pre_a=True, transposed=True, rec=(1, 64, 0, 0, 0, 1, 1, 64, 1, 0)),
    case(3, 107, 64, 32, 16, S=8, pad=4, dt="f32", pre_a=True, transposed=True, rec=(1, 64, 0, 0, 0, 1, 3, 128, 0, 1)),
    # K = 1 kernel: 1, 2 and 3 chunks, a one-row last chunk, 72 x 136 tiles, direct and split, bias on and off
    case(3, 20, 72, 136, 1, bias=True, rec=(3, 128, 0, 0, 0, 1, 1, 64, 1, 0)),
    case(5, 13, 72, 136, 1, rec=(3, 128, 0, 0, 0, 1, 1, 128, 1, 0)),
    case(3, 43, 72, 136, 1, bias=True, rec=(3, 128, 0, 0, 0, 1, 1, 192, 1, 0)),
    case(3, 43, 128, 128, 1, rec=(3, 128, 0, 0, 0, 1, 1, 192, 1, 0)),
    case(3, 171, 72, 136, 1, bias=True, rec=(3, 128, 0, 0, 0, 1, 2, 320, 0, 1)),
    case(3, 171, 72, 136, 1, knobs={"wgrad_cfg": 15}, rec=(3, 128, 0, 0, 0, 1, 2, 320, 0, 1)),
    case(3, 342, 72, 136, 1, bias=True, knobs={"wgrad_cfg": 16}, rec=(3, 128, 0, 0, 0, 1, 4, 320, 0, 1)),
    case(3, 171, 72, 136, 1, knobs={"wgrad_cfg": 14}, bias=True, rec=(1, 64, 0, 0, 0, 1, 5, 128, 0, 1)),
    # multi-tap kernel, every instantiation: K = KG taps in one run (wgrad_kg where the plan would cut them), T_A =
    # 57
    case(3, 57, 32, 32, 2, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 1, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 2, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 32, 2, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 3, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 4, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 32, 4, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 5, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 32, 5, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 24, 24, 6, pad=2, pre_b=True, knobs={"wgrad_kg": 6}, rec=(2, 32, 6, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 7, pad=3, knobs={"wgrad_kg": 7}, rec=(2, 32, 7, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 8, pad=3, knobs={"wgrad_kg": 8}, rec=(2, 32, 8, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 9, pad=4, bias=True, knobs={"wgrad_kg": 9}, rec=(2, 32, 9, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 10, pad=4, pre_b=True, knobs={"wgrad_kg": 10}, rec=(2, 32, 10, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 11, pad=5, knobs={"wgrad_kg": 11}, rec=(2, 32, 11, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 32, 32, 2, S=2, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 2, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 2, S=2, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 32, 2, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 3, S=2, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 4, S=2, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 32, 4, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 5, S=2, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 32, 5, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 24, 24, 6, S=2, pad=2, pre_b=True, knobs={"wgrad_kg": 6}, rec=(2, 32, 6, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 7, S=2, pad=3, knobs={"wgrad_kg": 7}, rec=(2, 32, 7, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 8, S=2, pad=3, knobs={"wgrad_kg": 8}, rec=(2, 32, 8, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 9, S=2, pad=4, bias=True, knobs={"wgrad_kg": 9}, rec=(2, 32, 9, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 10, S=2, pad=4, pre_b=True, knobs={"wgrad_kg": 10}, rec=(2, 32, 10, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 11, S=2, pad=5, knobs={"wgrad_kg": 11}, rec=(2, 32, 11, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 32, 32, 2, S=4, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 4, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 2, S=3, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 32, 2, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 3, S=4, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 4, S=3, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 32, 4, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 5, S=4, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 32, 5, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 24, 24, 6, S=3, pad=2, pre_b=True, knobs={"wgrad_kg": 6}, rec=(2, 32, 6, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 7, S=4, pad=3, knobs={"wgrad_kg": 7}, rec=(2, 32, 7, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 8, S=3, pad=3, knobs={"wgrad_kg": 8}, rec=(2, 32, 8, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 24, 24, 9, S=4, pad=4, bias=True, knobs={"wgrad_kg": 9}, rec=(2, 32, 9, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 10, S=3, pad=4, pre_b=True, knobs={"wgrad_kg": 10}, rec=(2, 32, 10, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 11, S=4, pad=5, knobs={"wgrad_kg": 11}, rec=(2, 32, 11, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 64, 2, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 64, 1, 1, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 2, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 64, 2, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 40, 72, 3, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 64, 3, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 4, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 64, 4, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 64, 64, 5, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 64, 5, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 40, 72, 6, pad=2, pre_b=True, knobs={"wgrad_kg": 6}, rec=(2, 64, 6, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 64, 64, 7, pad=3, knobs={"wgrad_kg": 7}, rec=(2, 64, 7, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 8, pad=3, knobs={"wgrad_kg": 8}, rec=(2, 64, 8, 1, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 64, 64, 2, S=2, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 64, 1, 2, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 2, S=2, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 64, 2, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 40, 72, 3, S=2, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 64, 3, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 4, S=2, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 64, 4, 2, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 64, 64, 5, S=2, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 64, 5, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 64, 2, S=4, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 64, 1, 4, 2, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 2, S=3, pre_b=True, knobs={"wgrad_kg": 2}, rec=(2, 64, 2, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 40, 72, 3, S=4, pad=1, knobs={"wgrad_kg": 3}, rec=(2, 64, 3, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 64, 4, S=3, pad=1, knobs={"wgrad_kg": 4}, rec=(2, 64, 4, 4, 1, 1, 6, 64, 0, 1)),
    case(3, 57, 64, 64, 5, S=4, pad=2, bias=True, knobs={"wgrad_kg": 5}, rec=(2, 64, 5, 4, 1, 1, 3, 64, 0, 1)),
    # multi-tap kernel: 1 to 4 chunks per split, a tap run cut short, the window at its limit, dil > 64, K >= 16 at
    # T_A = 65, the transposed form, groups, the 16-wave reduce
    case(3, 64, 8, 8, 11, pad=5, groups=16, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 1, 11, 1, 3, 64, 0, 1)),
    case(3, 128, 8, 8, 11, pad=5, groups=16, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 1, 11, 1, 3, 128, 0, 1)),
    case(3, 192, 8, 8, 11, pad=5, groups=16, bias=True, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 1, 11, 1, 3, 192, 0, 1)),
    case(3, 256, 8, 8, 11, pad=5, groups=16, knobs={"wgrad_kg": 1}, rec=(2, 32, 1, 1, 11, 1, 3, 256, 0, 1)),
    case(3, 249, 8, 8, 11, pad=5, groups=32, pre_b=True, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 1, 4, 1, 4, 192, 0, 1)),
    # many taps over long utterances with one row past each end in reach of the last tap: a one-row fault at an
    # utterance boundary here stays under a whole-tensor 1e-2
    case(3, 384, 8, 8, 41, pad=1, rec=(2, 32, 3, 1, 14, 1, 18, 64, 0, 1)),
    case(3, 384, 8, 8, 11, pad=5, groups=16, rec=(2, 32, 11, 1, 1, 1, 18, 64, 0, 1)),
    case(3, 121, 64, 64, 9, pad=4, knobs={"wgrad_kg": 8}, bias=True, rec=(2, 64, 8, 1, 2, 1, 6, 64, 0, 1)),
    case(3, 121, 32, 32, 9, pad=4, knobs={"wgrad_kg": 8}, rec=(2, 32, 8, 1, 2, 1, 6, 64, 0, 1)),
    case(3, 57, 32, 32, 7, S=2, pad=3, knobs={"wgrad_kg": 4}, rec=(2, 32, 4, 2, 2, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 64, 7, S=4, pad=3, knobs={"wgrad_kg": 4}, rec=(2, 64, 4, 4, 2, 1, 3, 64, 0, 1)),
    case(3, 57, 32, 32, 3, dil=32, pad=32, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 40, 3, dil=32, pad=32, pre_b=True, knobs={"wgrad_kg": 3}, rec=(2, 64, 3, 1, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 32, 32, 3, S=2, dil=32, pad=32, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 40, 3, S=2, dil=32, pad=32, pre_b=True, knobs={"wgrad_kg": 3},
         rec=(2, 64, 3, 2, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 32, 32, 3, S=4, dil=32, pad=32, knobs={"wgrad_kg": 3}, rec=(2, 32, 3, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 57, 64, 40, 3, S=4, dil=32, pad=32, pre_b=True, knobs={"wgrad_kg": 3},
         rec=(2, 64, 3, 4, 1, 1, 3, 64, 0, 1)),
    case(3, 121, 32, 32, 2, dil=65, pad=32, rec=(2, 32, 1, 1, 2, 1, 6, 64, 0, 1)),
    case(3, 65, 32, 32, 16, pad=8, bias=True, rec=(2, 32, 1, 1, 16, 1, 6, 64, 0, 1)),
    case(3, 65, 64, 64, 41, S=4, pad=20, pre_b=True, rec=(2, 64, 1, 4, 41, 1, 6, 64, 0, 1)),
    case(3, 64, 32, 32, 4, S=2, pad=1, pre_a=True, transposed=True, rec=(2, 32, 1, 2, 4, 1, 3, 64, 0, 1)),
    case(3, 121, 64, 32, 4, S=2, pad=1, pre_a=True, transposed=True, rec=(2, 64, 1, 2, 4, 1, 6, 64, 0, 1)),
    case(3, 121, 32, 16, 5, S=2, pad=2, groups=4, bias=True, pre_b=True, rec=(2, 32, 1, 2, 5, 1, 6, 64, 0, 1)),
    case(3, 64, 64, 64, 3, pad=1, groups=2, bias=True, rec=(2, 64, 1, 1, 3, 1, 3, 64, 0, 1)),
    case(36, 32, 24, 24, 16, pad=8, bias=True, rec=(2, 32, 2, 1, 8, 1, 36, 64, 0, 16)),
    case(36, 32, 32, 32, 16, pad=8, rec=(2, 32, 2, 1, 8, 1, 36, 64, 0, 16)),
]

# Every shipped instantiation and path of csrc/wgrad.hip, by hand from the source (see wgrad_check.reached for
# what each name means).
REQUIRED = set()
# wgrad_kernel<bf16_t | float | bx3_t>
for _dt in ("bf16", "f32", "x3"):
    REQUIRED |= {f"per_tap/{_dt}/{p}" for p in (
        "direct", "partials_one_split", "splits", "split_inside_utterance_one_row_tail", "partial_tile", "pre_b",
        "bias", "no_bias", "pad>T")}
for _dt in ("bf16", "f32"):
    REQUIRED |= {f"per_tap/{_dt}/{p}" for p in (
        "S2", "S3", "S4", "S8", "grouped_gpt1/bias", "gpt>1/bias", "transposed")}
# wgrad_k1_kernel: both exits of the double-buffered loop (1, 2, 3+ chunks)
REQUIRED |= {"k1/chunks/1", "k1/chunks/2", "k1/chunks/3", "k1/one_row_tail", "k1/partial_tile", "k1/direct",
             "k1/split", "k1/bias", "k1/no_bias"}
# wgrad_mt_kernel<TM, KG, SW>: the 51 instantiations of wgrad_mt_dispatch
REQUIRED |= {("mt", 32, kg, sw) for kg in range(1, 12) for sw in (1, 2, 4)}
REQUIRED |= {("mt", 64, kg, 1) for kg in range(1, 9)}
REQUIRED |= {("mt", 64, kg, sw) for kg in range(1, 6) for sw in (2, 4)}
REQUIRED |= {f"mt/chunks_per_split/{n}" for n in (1, 2, 3, 4)}  # every exit of the 2x-unrolled chunk loop
REQUIRED |= {"mt/last_chunk/57", "mt/last_chunk/1", "mt/short_last_run", "mt/window_limit/SW1",
             "mt/window_limit/SW2", "mt/window_limit/SW4", "mt/dil>64", "mt/S3", "mt/pre_a", "mt/pre_b", "mt/groups",
             "mt/bias/TM32", "mt/bias/TM64", "mt/partial_tile/TM32", "mt/partial_tile/TM64"}
# wgrad_reduce_kernel<16, 1> and <1, 4>
REQUIRED |= {"reduce/W16", "reduce/W1", "reduce/W16/ragged", "reduce/W1/ragged", "reduce/W16/bias", "reduce/W1/bias"}

# colsum_kernel<bf16_t | float>: C = 8, 40 (5 vectors per row do not divide 256), 256, 2048; one row, and one
# row past a block's rows_per_block (max(8 x (256 / (C / 8)), rows / 1024))
COLSUM = [WC.colsum_case(rows, C, dt) for dt in ("bf16", "f32")
          for C, rpb in ((8, 2048), (40, 408), (256, 64), (2048, 8)) for rows in (1, rpb + 1)]

_worst = {}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(c, m):
    """Both runs of the case on the GPU; copies every buffer back into m."""
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    a_buf, b_buf = m["a_buf"].cuda(), m["b_buf"].cuda()
    a, b = WC.a_view(c, a_buf), WC.b_view(c, b_buf)
    assert a.stride(1) == c["lda"] and b.stride(1) == c["ldb"]
    want = WC.record(c)
    for o in m["outs"]:
        dw_buf, ws_buf = o["dw_buf"].cuda(), o["ws_buf"].cuda()
        db_buf = o["db_buf"].cuda() if c["bias"] else None
        with WC.knobs(c):
            assert ops.conv1d_wgrad_plan(*WC.plan_args(c)[0], **WC.plan_args(c)[1]) == want
            rc = L.vo_conv1d_wgrad_bias(_ptr(a), c["lda"], c["T_A"], _ptr(b), c["ldb"], c["T_B"], c["B"], c["M"],
                                        c["N"], c["K"], c["S"], c["dil"], c["pad"], c["groups"], int(c["pre_a"]),
                                        int(c["pre_b"]), WC.SLOPE, WC.VO_DT[c["dt"]], _ptr(WC.dw_view(c, dw_buf)),
                                        _ptr(WC.db_view(c, db_buf)) if c["bias"] else None, _ptr(ws_buf),
                                        torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "vo_conv1d_wgrad_bias")
            got = ops.conv1d_wgrad_last_launch()
        assert got == want, (got, want)
        torch.cuda.synchronize()
        o["dw_buf"], o["ws_buf"] = dw_buf.cpu(), ws_buf.cpu()
        if c["bias"]:
            o["db_buf"] = db_buf.cpu()
    m["a_buf"], m["b_buf"] = a_buf.cpu(), b_buf.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_wgrad_edges(c):
    m = WC.make(c)
    ref = WC.reference(c, m)
    _run(c, m)
    ratio, rel = WC.verify(c, m, ref)
    route = {WC.PER_TAP: "per-tap " + c["dt"], WC.MULTI_TAP: "multi-tap", WC.K1: "K = 1"}[WC.record(c)["ROUTE"]]
    w = _worst.setdefault(route, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], rel)
    print(f"worst so far, {route}: error/bar {w[0]:.3e}, rel-L2 {w[1]:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", COLSUM, ids=[c["name"] for c in COLSUM])
def test_colsum_edges(c):
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    m = WC.colsum_make(c)
    x_buf = m["x_buf"].cuda()
    for o in m["outs"]:
        out_buf, ws_buf = o["out_buf"].cuda(), o["ws_buf"].cuda()
        rc = L.vo_colsum(_ptr(WC.colsum_view(c, x_buf)), c["rows"], c["C"], c["ld"], WC.VO_DT[c["dt"]],
                         _ptr(out_buf[WC.GUARD_N:]), _ptr(ws_buf), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "vo_colsum")
        torch.cuda.synchronize()
        o["out_buf"], o["ws_buf"] = out_buf.cpu(), ws_buf.cpu()
    m["x_buf"] = x_buf.cpu()
    WC.colsum_verify(c, m)


@pytest.mark.gpu
def test_rejected_wgrad_leaves_a_zero_record_on_the_gpu():
    """A real launch fills the record, the next refused call (M not a multiple of 8) zeroes it."""
    from visual_onoma_to_wave_amd import _lib, ops
    a = torch.zeros(2, 16, 64, dtype=torch.bfloat16, device="cuda")
    ops.conv1d_wgrad(a, a, 3, pad=1)
    assert ops.conv1d_wgrad_last_launch()["ROUTE"] == WC.PER_TAP
    ws = torch.zeros(1024, device="cuda")
    rc = _lib.lib().vo_conv1d_wgrad_bias(a.data_ptr(), 64, 16, a.data_ptr(), 64, 16, 2, 60, 64, 3, 1, 1, 1, 1, 0, 0,
                                         0.0, 1, ws.data_ptr(), None, ws.data_ptr(), None)
    assert rc == -1 and set(ops.conv1d_wgrad_last_launch().values()) == {0}
