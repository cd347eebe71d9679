"""Golden vectors for the repeat / consecutive augmentation, from the reference itself.

Runs only where the reference is mounted (``make_goldens.REF``).  It writes a temporary preprocessed directory of
seven seeded synthetic base utterances (1 to 8 katakana, 80-bin mels of at most 40 frames, gray strips 24 pixels high
saved as the RGB PNGs the reference's renderer saves) and runs the reference's own ``Preprocessor._augmentation`` over
them, once with the packaged ``augmentation:`` values (``cfg_a``) and once with ``first_consecutive: 2`` (``cfg_b``).
The reference is driven through ``object.__new__(Preprocessor)`` carrying only the attributes those methods read;
modules that ``preprocessor.py`` imports at its top and that are not installed get an empty stand-in in
``sys.modules`` (none of them is on the augmentation's path).  Nothing of the reference's text is here.

The utterances: a plain two-character text, a single character, a run of three at the END of the text, a run of three
in the middle, a run of three whose middle character has a ZERO duration, seven characters without a run
(``max_length`` itself) and eight characters (over ``max_length``: the reference writes no variant).

One case the reference does not survive as it stands: with ``first_consecutive >= 1`` its ``_augmentation`` adds the
``(frames, text)`` pair that ``_consecutiveaug`` returns to an integer and raises TypeError after the first file.  The
driver wraps the instance's ``_consecutiveaug`` so that the pair also adds as its first item; the files are still
written by the reference's own method, and the loop runs on as written.  The same wrappers record the order of the
calls, which is the order ``variants()`` must give.  No other case raised (``pos = 0`` crops a zero-width left part,
which PIL accepts).

Written, as data only, to augment.npz (flat arrays with offsets: one zip member per kind, so that the copies the
variants are made of deflate against each other):

    base_*      names, labels, texts; char_off (U + 1), dur int64, energy / kurtosis float64, width int32 (flat);
                frame_off (U + 1), mel (sum F, 80) float32; px_off (U + 1), strip_w (U), strip uint8 (flat, 24 rows each)
    var_*       the same for every file the reference wrote under either configuration, + var_src (its base)
    order_a/b   indices into var_* in the order the reference wrote them under cfg_a / cfg_b
    cfg_a/b     max_length, repeat_num, consecutive_num, first_consecutive
    cpos_text, cpos_pos   strings and the reference's _get_consecutive_pos answer (-1: None)

    python tests/golden/make_goldens_augment.py
"""

import importlib
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

H, N_MELS, FONT, FS = 24, 80, "ipaexg", 24
CFG_A = {"max_length": 7, "repeat_num": 3, "consecutive_num": 5, "first_consecutive": 0}
CFG_B = dict(CFG_A, first_consecutive=2)
# (label, stem, text, durations or None for seeded ones)
BASES = [
    ("drum", "drum-a1-001", "ワン", None),
    ("cup1", "cup1-a1-002", "カ", None),
    ("maracas", "maracas-a1-003", "ガリリリ", None),
    ("bells5", "bells5-a1-004", "ジーーーン", None),
    ("whistle3", "whistle3-a1-005", "ピーーーッ", [4, 3, 0, 6, 2]),
    ("clock1", "clock1-a1-006", "チリンチリンチ", None),
    ("shaver", "shaver-a1-007", "ガラガラガラガラ", None),
]
CPOS = ["", "ア", "アア", "アイ", "アイウ", "アアイ", "アイイ", "アアア", "アアアイ", "イアアア", "イアアアイ", "アアアア", "アアアアイ",
        "イアアアア", "イウアアアアエ", "アアアアア", "アアアアアイ", "イアアアアア", "イアアアアアウ", "アアイイ", "アアイイイ", "アアアイイ",
        "アアアイイイ", "アアイイイウウウ", "アイアイアイ", "アアイアアイアアア", "アアイイウウ", "イイアアアイイ", "ーーー", "ピーーー", "ピーーーッ",
        "ガリリリ", "ジーーーン", "アイウエオアアア", "アイウエアアアオ", "アアアイウエオ", "アイアアアアイア", "アアアアイイイイ", "アイイイイアアア",
        "ンンンンンンン", "アイウエオカキ"]


def import_preprocessor():
    import make_goldens as MG
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(MG.REF, "scripts"))
    for name in ("tqdm", "librosa", "tgt", "torchaudio", "joblib", "sklearn", "sklearn.preprocessing"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(tqdm=None, Parallel=None, delayed=None, StandardScaler=None)
            sys.modules[name] = m
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], m)
    from preprocessor.preprocessor import Preprocessor
    return Preprocessor


class _Pair(tuple):
    """What ``_consecutiveaug`` returns, that also adds to an integer as its first item (see the docstring)."""

    def __radd__(self, other):
        return other + self[0]


def make_bases(rng):
    out = []
    for label, stem, text, dur in BASES:
        n = len(text)
        dur = np.asarray(dur if dur is not None else rng.integers(1, 6, size=n), np.int64)
        assert int(dur.sum()) <= 40
        width = rng.integers(5, 41, size=n).astype(np.int32)
        out.append({
            "name": f"{FONT}_{FS}pt_{stem}", "label": label, "stem": stem, "text": text, "dur": dur, "width": width,
            "energy": rng.standard_normal(n), "kurtosis": rng.standard_normal(n),
            "mel": (rng.integers(-400, 400, size=(int(dur.sum()), N_MELS)) / 8).astype(np.float32),
            "strip": rng.integers(0, 256, size=(H, int(width.sum()))).astype(np.uint8)})
    return out


def write_base(root, u):
    from PIL import Image
    for sub, a in (("duration", u["dur"]), ("energy", u["energy"]), ("kurtosis", u["kurtosis"]), ("mel", u["mel"]),
                   ("image/width", u["width"])):
        np.save(root / sub / u["label"] / f"{u['name']}.npy", a)
    Image.fromarray(np.repeat(u["strip"][:, :, None], 3, axis=2)).save(root / "image/png" / u["label"] / f"{u['name']}.png")


def read_variant(root, label, name):
    from PIL import Image
    ld = lambda sub: np.load(root / sub / label / f"{name}.npy")  # noqa: E731
    with Image.open(root / "image/png" / label / f"{name}.png") as im:
        strip = np.asarray(im.convert("L"), dtype=np.uint8)
    info = None
    for split in ("train", "val_test"):
        p = root / "intermediate/info" / split / label / f"{name}.txt"
        if p.exists():
            info = p.read_text(encoding="utf-8")
    return {"name": name, "text": info.split("|")[4], "dur": ld("duration"), "energy": ld("energy"),
            "kurtosis": ld("kurtosis"), "mel": ld("mel"), "width": ld("image/width"), "strip": strip}


def run_reference(Preprocessor, bases, cfg):
    """-> [(base index, variant dict), ...] in the order the reference wrote them."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        for u in bases:
            for sub in ("duration", "energy", "kurtosis", "mel", "image/width", "image/png", "intermediate/info/train",
                        "intermediate/info/val_test"):
                (root / sub / u["label"]).mkdir(parents=True, exist_ok=True)
            write_base(root, u)
        p = object.__new__(Preprocessor)
        p.path_preprocessed, p.path_font, p.im_fontsize, p.valtest_id = root, Path(f"{FONT}.ttf"), FS, []
        p.aug_maxlen, p.aug_repeatnum = cfg["max_length"], cfg["repeat_num"]
        p.aug_chara_consecutive_num, p.aug_first_consecutive = cfg["consecutive_num"], cfg["first_consecutive"]
        written = []

        def repeataug(repeat_num, label, basename, savename, text):
            written.append(savename)
            return Preprocessor._repeataug(p, repeat_num, label, basename, savename, text)

        def consecutiveaug(num, pos, label, basename, savename, text):
            written.append(savename)
            return _Pair(Preprocessor._consecutiveaug(p, num, pos, label, basename, savename, text))

        p._repeataug, p._consecutiveaug = repeataug, consecutiveaug
        for i, u in enumerate(bases):
            del written[:]
            p._augmentation(u["label"], f"{u['stem']}|x|{u['text']}|x|x|x\n")
            out += [(i, read_variant(root, u["label"], name)) for name in written]
    return out


def pack(prefix, items):
    """Flat arrays with offsets for a list of utterance dicts."""
    cat = lambda k, dt: np.concatenate([np.asarray(u[k]).reshape(-1) for u in items]).astype(dt)  # noqa: E731
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)  # noqa: E731
    for u in items:  # what is stored is what the reference's files hold, dtype included
        assert u["dur"].dtype == np.int64 and u["energy"].dtype == np.float64 and u["kurtosis"].dtype == np.float64
        assert u["width"].dtype == np.int32 and u["mel"].dtype == np.float32 and u["mel"].shape[1] == N_MELS
        assert u["strip"].shape[0] == H
    return {
        f"{prefix}_names": np.array([u["name"] for u in items]), f"{prefix}_texts": np.array([u["text"] for u in items]),
        f"{prefix}_char_off": off([len(u["dur"]) for u in items]), f"{prefix}_dur": cat("dur", np.int64),
        f"{prefix}_energy": cat("energy", np.float64), f"{prefix}_kurtosis": cat("kurtosis", np.float64),
        f"{prefix}_width": cat("width", np.int32), f"{prefix}_frame_off": off([u["mel"].shape[0] for u in items]),
        f"{prefix}_mel": np.concatenate([u["mel"] for u in items]).astype(np.float32),
        f"{prefix}_px_off": off([u["strip"].size for u in items]),
        f"{prefix}_strip_w": np.array([u["strip"].shape[1] for u in items], np.int32), f"{prefix}_strip": cat("strip", np.uint8)}


def main():
    Preprocessor = import_preprocessor()
    bases = make_bases(np.random.default_rng(468622))
    run_a, run_b = run_reference(Preprocessor, bases, CFG_A), run_reference(Preprocessor, bases, CFG_B)
    union, index = [], {}
    orders = []
    for run in (run_a, run_b):
        order = []
        for src, v in run:
            if v["name"] in index:  # written under both configurations: the same file
                w = union[index[v["name"]]][1]
                assert all(np.array_equal(v[k], w[k]) for k in v if k != "name") and v["text"] == w["text"]
            else:
                index[v["name"]] = len(union)
                union.append((src, v))
            order.append(index[v["name"]])
        orders.append(np.asarray(order, np.int64))
    p = Preprocessor.__new__(Preprocessor)
    cpos = [p._get_consecutive_pos(s) for s in CPOS]
    arrays = dict(pack("base", bases), **pack("var", [v for _, v in union]))
    arrays.update(base_labels=np.array([u["label"] for u in bases]), var_src=np.array([s for s, _ in union], np.int64),
                  order_a=orders[0], order_b=orders[1],
                  cfg_a=np.array(list(CFG_A.values()), np.int64), cfg_b=np.array(list(CFG_B.values()), np.int64),
                  cpos_text=np.array(CPOS), cpos_pos=np.array([-1 if c is None else c for c in cpos], np.int64))
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", os.path.relpath(path, REPO), os.path.getsize(path), "bytes;", len(run_a), "+", len(union) - len(run_a),
          "variants;", sum(c is not None for c in cpos), "of", len(CPOS), "strings with a run")


if __name__ == "__main__":
    main()
