"""Do two builds of the library plan every weight-gradient call alike?  Host only, no GPU.

  python tools/probes/wgrad_plan_sweep.py compare LIB_A LIB_B OUT.json [--shapes FILE ...]

For each library and each knob setting a child process loads the library by path (ctypes, not the package's
bindings: the two builds may differ in ABI version), walks the grid below through vo_conv1d_wgrad_plan and
vo_conv1d_wgrad_workspace_size and writes one SHA-256 per (dtype, bias, B, T_A) block over (return code, the 12
record fields, the workspace size) of every combination, with the count of refused ones.  The parent compares the
digests block by block.  Settings: the defaults and every knob value the weight gradient still reads.

The edge matrix (tests/test_gpu_wgrad_edges.CASES) is walked under every setting and under each case's own knobs.
--shapes: outputs of `tools/probes/wgrad_shapes.py train` and `... gan` (every weight-gradient call of a C4 / C5
step, one tuple per line; wgrad_shapes_probe.py lists the C5 step only and prints another format), walked the same
way.
"""

import ast
import concurrent.futures
import ctypes
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BS, TS = (1, 3, 16, 36), (1, 12, 57, 64, 65, 121, 384, 8192)
MNS = (8, 24, 32, 40, 64, 72, 136, 1024)
KS, SS, DILS, GROUPS = (1, 2, 3, 5, 7, 9, 11, 16, 41), (1, 2, 3, 4, 8), (1, 3, 32, 65), (1, 2, 4, 16)
SETTINGS = [{}] + [{"wgrad_cfg": v} for v in (12, 13, 14, 15, 16)] + [{"wgrad_mt": v} for v in (1, 2)] + \
           [{"wgrad_kg": v} for v in range(1, 12)]
KNOBS = ("wgrad_cfg", "wgrad_mt", "wgrad_kg")
NREC = 12


def load(path):
    L = ctypes.CDLL(path)
    L.vo_conv1d_wgrad_plan.restype = ctypes.c_int
    L.vo_conv1d_wgrad_plan.argtypes = [ctypes.c_int] * 14 + [ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    L.vo_conv1d_wgrad_workspace_size.restype = ctypes.c_int64
    L.vo_conv1d_wgrad_workspace_size.argtypes = [ctypes.c_int] * 6
    L.vo_tune.restype = ctypes.c_int
    L.vo_tune.argtypes = [ctypes.c_char_p, ctypes.c_int]
    return L


def tune(L, knobs):
    for k in KNOBS:
        assert L.vo_tune(k.encode(), int(knobs.get(k, 0))) == 0, (k, knobs)


def edge_calls():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    from test_gpu_wgrad_edges import CASES
    from wgrad_check import VO_DT
    return [((c["B"], c["T_A"], c["T_B"], c["M"], c["N"], c["K"], c["S"], c["dil"], c["pad"], c["groups"],
              int(c["pre_a"]), int(c["pre_b"]), VO_DT[c["dt"]], int(c["bias"])), c["knobs"]) for c in CASES]


def shape_calls(files):
    """The calls a wgrad_shapes.py output lists; the prologue flag does not say which operand, so every variant."""
    out = set()
    for f in files:
        for line in open(f):
            m = re.search(r"\('(bfloat16|float32)', .*\)\s*$", line)
            if not m:
                continue
            dt, a, b, K, S, dil, pad, groups, tr, pre, bias, split = ast.literal_eval(m.group(0).strip())
            dtype = 1 if dt == "bfloat16" else 2 if split else 0
            M, N = a[-1] // groups, b[-1] // groups
            B, T_A, T_B = a[0] * (a[1] if len(a) == 4 else 1), a[-2], b[-2]
            for pa, pb in ((0, 0), (0, 1), (1, 0), (1, 1)) if pre else ((0, 0),):
                out.add((B, T_A, T_B, M, N, K, S, dil, pad, groups, pa, pb, dtype, int(bool(bias))))
    return sorted(out)


def child(lib_path, setting, shapes, out_path):
    L = load(lib_path)
    rec = (ctypes.c_int32 * NREC)()
    plan, wsz = L.vo_conv1d_wgrad_plan, L.vo_conv1d_wgrad_workspace_size
    res = {"blocks": {}, "compared": 0, "refused": 0}

    def one(h, args):
        rc = plan(*args, rec, NREC)
        res["compared"] += 1
        res["refused"] += rc != 0
        h.update(b"%d|%s|%d;" % (rc, bytes(rec), wsz(args[0], args[1], args[3], args[4], args[5], args[9])))

    tune(L, setting)
    for dtype, bias, B, T in itertools.product((0, 1, 2), (0, 1), BS, TS):
        h = hashlib.sha256()
        for M, N, K, S, dil, g in itertools.product(MNS, MNS, KS, SS, DILS, GROUPS):
            one(h, (B, T, (T - 1) * S + dil * (K - 1) + 1, M, N, K, S, dil, 0, g, 0, 0, dtype, bias))
        res["blocks"][f"grid dtype={dtype} bias={bias} B={B} T_A={T}"] = h.hexdigest()
    edges = edge_calls()
    for name, calls in (("edge", [a for a, _ in edges]), ("step", shapes)):
        for i, args in enumerate(calls):
            h = hashlib.sha256()
            one(h, args)
            res["blocks"][f"{name} {i} {args}"] = h.hexdigest()
    if not setting:  # once: each edge case under its own knobs
        for i, (args, kn) in enumerate(edges):
            tune(L, kn)
            h = hashlib.sha256()
            one(h, args)
            res["blocks"][f"edge-own-knobs {i} {args} {kn}"] = h.hexdigest()
        tune(L, {})
    json.dump(res, open(out_path, "w"))


def compare(lib_a, lib_b, out_json, shape_files):
    shapes = shape_calls(shape_files)
    total = {"libraries": [lib_a, lib_b], "settings": [], "compared": 0, "refused": 0, "mismatched_blocks": [],
             "step_shapes": len(shapes)}
    with tempfile.TemporaryDirectory() as tmp:
        cmds = [[sys.executable, __file__, "child", lib, json.dumps(s), json.dumps(shapes),
                 os.path.join(tmp, f"{tag}{si}.json")]
                for si, s in enumerate(SETTINGS) for tag, lib in (("a", lib_a), ("b", lib_b))]
        # one child per CPU, 16 at the most; a worker starts the next child as soon as its own has ended
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
            assert all(rc == 0 for rc in pool.map(lambda c: subprocess.run(c).returncode, cmds))
        results = [[json.load(open(os.path.join(tmp, f"{t}{si}.json"))) for t in "ab"] for si in range(len(SETTINGS))]
    for s, (ra, rb) in zip(SETTINGS, results):
        bad = [k for k in ra["blocks"] if ra["blocks"][k] != rb["blocks"].get(k)]
        assert ra["blocks"].keys() == rb["blocks"].keys()
        total["settings"].append({"knobs": s, "compared": ra["compared"], "refused_a": ra["refused"],
                                  "refused_b": rb["refused"], "mismatched_blocks": len(bad)})
        total["compared"] += ra["compared"]
        total["refused"] += ra["refused"]
        total["mismatched_blocks"] += [f"{s}: {k}" for k in bad]
    json.dump(total, open(out_json, "w"), indent=1)
    print(json.dumps({k: total[k] for k in ("compared", "refused", "step_shapes")}),
          "mismatched blocks:", len(total["mismatched_blocks"]))
    return 1 if total["mismatched_blocks"] else 0


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], json.loads(sys.argv[3]), [tuple(x) for x in json.loads(sys.argv[4])], sys.argv[5])
    else:
        files = sys.argv[sys.argv.index("--shapes") + 1:] if "--shapes" in sys.argv else []
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4], files))
