"""Golden vectors for the corpus statistics, from the reference itself.

Runs only where the reference is mounted (``make_goldens.REF``).  The reference is loaded as
``make_goldens_augment.import_preprocessor`` loads it, and its own ``Preprocessor._remove_outlier`` is applied to
the energy and the kurtosis array of every file that tests/golden/augment.npz already holds: the 7 base utterances
and the 53 variants the reference's ``_augmentation`` wrote from them under its two configurations.  Each file is
taken twice: as the reference wrote it (float64, "f64") and rounded to float32 and back ("f32"), which is what
``DeviceCorpus`` packs and ``to_device``'s ``.float()`` gives the model; the device statistics are those of the
"f32" arrays.  sklearn is importable where this was run, so ``StandardScaler.partial_fit`` over the kept arrays in
file order (the loop of ``build_from_path``, preprocessor.py:114-127; arrays that keep nothing are skipped as there)
gives the stored ``mean_`` / ``scale_``.  Nothing of the reference's text is here.

A handful of hand-made arrays go through the same ``_remove_outlier``: one value, all values equal, 2 to 5 values
(the virtual index of a quartile has the fractional part 0, .25, .5 and .75), quartiles that coincide while distinct
outliers exist, a value exactly on the upper fence (the comparison is strict: it is dropped), seeded float32 draws
of 4, 64 and 65 values whose interpolation rounds, and one array with a far outlier on each side.

Written, as data only, to corpus_stats.npz:

    names                        the 60 file names, bases first, then the variants in augment.npz's order
    {feature}_{prec}_kept(_off)  what _remove_outlier keeps of each file, flat float64 with offsets (61)
    {feature}_{prec}_scaler      StandardScaler's mean_[0], scale_[0]
    hand(_off), hand_kept(_off), hand_names

    python tests/golden/make_goldens_stats.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)


def hand_arrays():
    rng = np.random.default_rng(113144)
    f32 = lambda n: rng.standard_normal(n).astype(np.float32).astype(np.float64)  # noqa: E731
    return [
        ("one", np.array([0.5])),
        ("equal", np.full(6, -1.25)),
        ("two", np.array([0.25, -3.0])),
        ("three", np.array([2.0, -1.0, 0.5])),
        ("four", np.array([0.1, 0.7, -0.3, 0.2]).astype(np.float32).astype(np.float64)),
        ("five", np.array([1.0, 9.0, 2.0, 4.0, 3.0])),
        ("quartiles_coincide", np.array([5.0, 0.0, 5.0, 5.0, 5.0, 9.0, 5.0, 5.0])),
        ("on_the_upper_fence", np.array([13.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])),
        ("draw4", f32(4)),
        ("draw64", f32(64)),
        ("draw65", f32(65)),
        ("far_outliers", np.concatenate([f32(30), [40.0, -55.0]])),
    ]


def flat(arrays):
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
    return np.concatenate([np.asarray(a, np.float64) for a in arrays] + [np.zeros(0)]), off


def main():
    from sklearn.preprocessing import StandardScaler
    from make_goldens_augment import import_preprocessor
    Preprocessor = import_preprocessor()
    p = object.__new__(Preprocessor)
    g = np.load(os.path.join(HERE, "augment.npz"))
    files = {"energy": [], "kurtosis": []}
    names = []
    for prefix in ("base", "var"):
        off = g[f"{prefix}_char_off"]
        names += [str(s) for s in g[f"{prefix}_names"]]
        for f in files:
            files[f] += [g[f"{prefix}_{f}"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    assert len(names) == 60 and all(a.dtype == np.float64 for a in files["energy"] + files["kurtosis"])
    out = {"names": np.array(names)}
    for f, arrays in files.items():
        for prec, cast in (("f64", lambda a: a), ("f32", lambda a: a.astype(np.float32).astype(np.float64))):
            kept = [p._remove_outlier(cast(a)) for a in arrays]
            scaler = StandardScaler()
            for k in kept:
                if len(k) > 0:
                    scaler.partial_fit(k.reshape(-1, 1))
            out[f"{f}_{prec}_kept"], out[f"{f}_{prec}_kept_off"] = flat(kept)
            out[f"{f}_{prec}_scaler"] = np.array([scaler.mean_[0], scaler.scale_[0]], np.float64)
    hand = hand_arrays()
    out["hand_names"] = np.array([n for n, _ in hand])
    out["hand"], out["hand_off"] = flat([a for _, a in hand])
    out["hand_kept"], out["hand_kept_off"] = flat([p._remove_outlier(a) for _, a in hand])
    path = os.path.join(HERE, "corpus_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, REPO), os.path.getsize(path), "bytes;", len(names), "files;",
          {k: int(v[-1]) for k, v in out.items() if k.endswith("_kept_off")})


if __name__ == "__main__":
    main()
