"""Timeline of one tile of the MRF stage-0 plane conv (csrc/conv_plane.hip) from s_memtime stamps.
Diagnostic library built here (never the product one):

    hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 \
        -DVO_CPL_STAMPS visual_onoma_to_wave_amd/csrc/conv_plane.hip visual_onoma_to_wave_amd/csrc/vo_runtime.cpp \
        -o tools/probes/build/libcpl_stamps.so
    python tools/probes/cpl_stamps.py [k d [B]]

Prints, for workgroups 0-15 (median over waves and workgroups; every workgroup is one tile), the cycles of the
prologue (first loads to the first barrier), each 32-channel chunk, the row-tile-major part of the last chunk with
the epilogues under it, and the last row tile's epilogue.  Ideal chunk: K taps x 64 MFMAs x 16 cycles = 1,024 K.
The call carries res1 and res2 (a chain's last c2)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_onoma_to_wave_amd import ops  # noqa: E402

NSTW, NPT, NC = 16, 16, 8


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    d = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    L = ctypes.CDLL(os.environ.get("CPL_LIB", os.path.join(ROOT, "tools/probes/build/libcpl_stamps.so")))
    C, T = 256, 4096
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16)
    r = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16)
    y = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16)
    b = torch.randn(C, device="cuda", generator=g) * 0.1
    w = ops.pack_conv_weight(torch.randn(C, C, k, device="cuda", generator=g) / (C * k) ** 0.5, torch.bfloat16)
    desc, _, _, _ = ops._conv1d_desc(x, w, b, Co=C, K=k, dil=d, pad=d * (k - 1) // 2, pre_act=ops.ACT_LRELU,
                                     pre_slope=0.1, out=y, res1=r, res2=y, out_scale=1 / 3, variant=1)
    buf = (ctypes.c_ulonglong * (NSTW * 4 * NPT))()
    fn = L.vo_cpl_stamps
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    for _ in range(3):  # warm clocks; keep the last
        assert fn(ctypes.byref(desc), ctypes.cast(buf, ctypes.c_void_p)) == 0
    st = np.frombuffer(buf, dtype=np.uint64).astype(np.int64).reshape(NSTW, 4, NPT)
    names = ["prologue"] + [f"chunk {c}" for c in range(NC - 1)] + ["chunk 7, piece-major part", "row-tile-major part",
                                                                   "last epilogue"]
    idx = [(0, 1)] + [(2 + c, 3 + c) for c in range(NC - 1)] + [(2 + NC - 1, 2 + NC), (2 + NC, 3 + NC), (3 + NC, 4 + NC)]
    tot = np.median((st[..., 4 + NC] - st[..., 0]).ravel())
    print(f"k={k} d={d} B={B}: median tile {tot:.0f} cycles (MFMA {NC * k * 1024}; chunk {k * 1024})")
    for nm, (i0, i1) in zip(names, idx):
        v = (st[..., i1] - st[..., i0]).ravel()
        print(f"  {nm:28s} median {np.median(v):8.0f}  p10 {np.percentile(v, 10):8.0f}  p90 {np.percentile(v, 90):8.0f}")


if __name__ == "__main__":
    main()
