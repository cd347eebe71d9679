"""Do two checkouts compute the same weight gradients, bit for bit?

  python tools/probes/wgrad_bits.py ROOT OUT.json    (once per checkout, ROOT = its root; then compare the files)

Every case of ROOT/tests/test_gpu_wgrad_edges.CASES through ROOT's package and library on the seeded inputs of
wgrad_check.make; SHA-256 of dW and db per case."""
import hashlib
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path[:0] = [root, os.path.join(root, "tests")]
import torch  # noqa: E402
import test_gpu_wgrad_edges as T  # noqa: E402
import wgrad_check as WC  # noqa: E402

out = {}
for c in T.CASES:
    m = WC.make(c)
    T._run(c, m)
    o = m["outs"][0]
    h = {"dW": hashlib.sha256(WC.dw_view(c, o["dw_buf"]).contiguous().numpy().tobytes()).hexdigest()}
    if c["bias"]:
        h["db"] = hashlib.sha256(WC.db_view(c, o["db_buf"]).contiguous().numpy().tobytes()).hexdigest()
    out[c["name"]] = h
import visual_onoma_to_wave_amd  # noqa: E402
assert os.path.abspath(visual_onoma_to_wave_amd.__file__).startswith(root), visual_onoma_to_wave_amd.__file__
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(len(out), "cases hashed from", root)
