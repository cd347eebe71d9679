"""Per-call time of each weight-gradient kernel, to compare two checkouts.

  python tools/probes/wgrad_route_time.py ROOT OUT.json    (alternately on the two checkouts, ROOT = its root)

Microseconds per vo_conv1d_wgrad_bias call through ROOT's package and library, one shape per kernel (the 51
multi-tap instantiations, the three per-tap compute types at the C4 encoder's 384-row shapes and at 16384 rows,
two step shapes, the K = 1 kernel): 20 warm-up calls, then 5 timings of 100 back-to-back calls between two events."""
import json
import os
import statistics
import sys

root = os.path.abspath(sys.argv[1])
sys.path[:0] = [root, os.path.join(root, "tests")]
import torch  # noqa: E402
from visual_onoma_to_wave_amd import _lib, ops  # noqa: E402

L = _lib.lib()
DT = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "x3": (2, torch.float32)}
SHAPES = []
for tm in (32, 64):
    for sw in (1, 2, 4):
        for kg in range(1, (11 if tm == 32 else 8 if sw == 1 else 5) + 1):
            SHAPES.append(dict(name=f"mt<{tm},{kg},{sw}>", B=16, T_A=2048, M=tm, N=tm, K=kg, S=sw, dt="bf16", kg=kg))
# the FFN w_1 weight gradient of the C4 decoder (k = 9: 5 + 4 taps) and the k = 41 stride-2 MSD layer
SHAPES.append(dict(name="mt ffn 256x1024 k9", B=16, T_A=512, M=1024, N=256, K=9, S=1, dt="bf16", pad=4))
SHAPES.append(dict(name="mt msd k41 s2 g4", B=16, T_A=2048, M=32, N=8, K=41, S=2, dt="bf16", pad=20, groups=4))
for dt in ("bf16", "f32", "x3"):  # per-tap, 384 rows in all (one chunk per split, direct) and a long one (splits + reduce)
    SHAPES.append(dict(name=f"per-tap {dt} 384 rows 256x256 k9", B=16, T_A=24, M=256, N=256, K=9, S=1, dt=dt, pad=4, mt=1))
    SHAPES.append(dict(name=f"per-tap {dt} 384 rows 256x1024 k1", B=16, T_A=24, M=1024, N=256, K=1, S=1, dt=dt, mt=1, cfg=14))
    SHAPES.append(dict(name=f"per-tap {dt} 16384 rows 128x128 k3", B=16, T_A=1024, M=128, N=128, K=3, S=1, dt=dt, pad=1, mt=1))
SHAPES.append(dict(name="k1 256x1024", B=16, T_A=512, M=1024, N=256, K=1, S=1, dt="bf16"))

out = {}
for s in SHAPES:
    vo_dt, tdt = DT[s["dt"]]
    B, T_A, M, N, K, S = (s[k] for k in ("B", "T_A", "M", "N", "K", "S"))
    pad, G = s.get("pad", 0), s.get("groups", 1)
    T_B = (T_A - 1) * S + (K - 1) + 1 - 2 * pad
    torch.manual_seed(1)
    a = torch.randn(B, T_A, G * M, device="cuda").to(tdt)
    b = torch.randn(B, T_B, G * N, device="cuda").to(tdt)
    L.vo_tune(b"wgrad_kg", s.get("kg", 0))
    L.vo_tune(b"wgrad_mt", s.get("mt", 0))
    L.vo_tune(b"wgrad_cfg", s.get("cfg", 0))
    rec = ops.conv1d_wgrad_plan(B, T_A, T_B, M, N, K, S=S, dil=1, pad=pad, groups=G, pre_a=False, pre_b=False,
                                dtype=vo_dt, with_bias=False)
    ws = torch.empty(int(L.vo_conv1d_wgrad_workspace_size(B, T_A, M, N, K, G)) // 4 + 64, device="cuda")
    dw = torch.empty(G * M, N, K, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        rc = L.vo_conv1d_wgrad_bias(a.data_ptr(), G * M, T_A, b.data_ptr(), G * N, T_B, B, M, N, K, S, 1, pad, G, 0, 0,
                                    0.1, vo_dt, dw.data_ptr(), None, ws.data_ptr(), st)
        assert rc == 0, (s, rc)

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 10.0)
    out[s["name"]] = dict(us=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2),
                          record=[rec[k] for k in ("ROUTE", "TM", "KG", "SW", "splits", "direct")])
    for k in (b"wgrad_kg", b"wgrad_mt", b"wgrad_cfg"):
        L.vo_tune(k, 0)
import visual_onoma_to_wave_amd  # noqa: E402
assert os.path.abspath(visual_onoma_to_wave_amd.__file__).startswith(root)
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(len(out), "shapes timed from", root)
