"""A numpy model of the augmentation's index maps (include/vonoma.h, vo_augment_batch) and the
golden corpus as ``Dataset.__getitem__`` dicts.  Written from the statement of the maps, not from the kernel: index
arrays built once per row and fancy indexing, where the kernel decides per element."""

import json
import os

import numpy as np

from helpers import DATA, golden

OK, BAD_ROW, CHARS_OVER, FRAMES_OVER = 0, 1, 2, 3
CFG_KEYS = ("max_length", "repeat_num", "consecutive_num", "first_consecutive")

_cache = {}


def symbol_ids():
    from visual_onoma_to_wave_amd.utils.symbols import get_symbols
    return get_symbols(DATA)


def _items(g, prefix, audiotypes, sym):
    out = []
    co, fo, po = g[f"{prefix}_char_off"], g[f"{prefix}_frame_off"], g[f"{prefix}_px_off"]
    for u in range(len(co) - 1):
        c, f = slice(co[u], co[u + 1]), slice(fo[u], fo[u + 1])
        w = int(g[f"{prefix}_strip_w"][u])
        out.append({"id": str(g[f"{prefix}_names"][u]), "audiotype": audiotypes[u],
                    "text": np.array([sym[t] for t in str(g[f"{prefix}_texts"][u])]),
                    "text_str": str(g[f"{prefix}_texts"][u]), "mel": g[f"{prefix}_mel"][f],
                    "energy": g[f"{prefix}_energy"][c], "kurtosis": g[f"{prefix}_kurtosis"][c],
                    "duration": g[f"{prefix}_dur"][c],
                    "image": (g[f"{prefix}_strip"][po[u]:po[u + 1]].reshape(-1, w), g[f"{prefix}_width"][c]),
                    "event_image_feature": None})
    return out


def load():
    """-> dict: bases, variants (lists of ``Dataset.__getitem__`` dicts + ``text_str``; a variant also has ``src``),
    order_a / order_b (indices into variants, the reference's write order), cfg_a / cfg_b, cpos [(text, pos or
    None)].  Loaded once; the arrays are shared and must not be written."""
    if not _cache:
        g = {k: v for k, v in golden("augment").items()}
        with open(os.path.join(DATA, "audiotype.json")) as f:
            amap = json.load(f)
        sym = symbol_ids()
        base_at = [amap[str(lab)] for lab in g["base_labels"]]
        bases = _items(g, "base", base_at, sym)
        variants = _items(g, "var", [base_at[s] for s in g["var_src"]], sym)
        for v, s in zip(variants, g["var_src"]):
            v["src"] = int(s)
        _cache.update(bases=bases, variants=variants, order_a=g["order_a"].tolist(), order_b=g["order_b"].tolist(),
                      cfg_a=dict(zip(CFG_KEYS, g["cfg_a"].tolist())), cfg_b=dict(zip(CFG_KEYS, g["cfg_b"].tolist())),
                      cpos=[(str(t), None if p < 0 else int(p)) for t, p in zip(g["cpos_text"], g["cpos_pos"])])
    return _cache


def sigma(n, pos, m, r):
    """Base character of each of the (n + m) r output characters."""
    jp = np.arange((n + m) * r) % (n + m)
    return np.where(jp < pos, jp, np.where(jp <= pos + m, pos, jp - m))


def phi(d, pos, m_mel, r):
    """Base frame of each of the (F + m_mel d[pos]) r output frames."""
    d = np.asarray(d, np.int64)
    s, dp, F = int(d[:pos].sum()), int(d[pos]), int(d.sum())
    F1 = F + m_mel * dp
    fp = np.arange(F1 * r) % max(F1, 1)
    mid = (fp >= s) & (fp < s + (m_mel + 1) * dp)
    return np.where(fp < s, fp, np.where(mid, s + (fp - s) % max(dp, 1), fp - m_mel * dp))


def model_row(u, pos, m, m_mel, r):
    """The variant ``(pos, m, m_mel, r)`` of base dict ``u`` as a ``Dataset.__getitem__`` dict (no id)."""
    strip, w = u["image"]
    sg, ph = sigma(len(u["text"]), pos, m, r), phi(u["duration"], pos, m_mel, r)
    col = np.concatenate([[0], np.cumsum(w)])
    cols = np.concatenate([np.arange(col[c], col[c + 1]) for c in sg] + [np.zeros(0, np.int64)]).astype(np.int64)
    return {"audiotype": u["audiotype"], "text": u["text"][sg], "mel": u["mel"][ph],
            "energy": None if u["energy"] is None else u["energy"][sg],
            "kurtosis": None if u["kurtosis"] is None else u["kurtosis"][sg], "duration": u["duration"][sg],
            "image": (strip[:, cols], w[sg]), "event_image_feature": None}


def layout(strip, widths, cell, margin, W_out):
    """``glyph_batch_kernel``'s layout of one strip -> (H, W_out) float32, for widths above the cell too: pleft is C's
    truncating (cell - len) / 2 + (cell - len) % 2, and the cell shows columns [-pleft, -pleft + cell) of the
    character."""
    H = strip.shape[0]
    px = np.full((H, W_out), 255, np.uint8)
    start = 0
    for j, ln in enumerate(int(v) for v in widths):
        dlt = cell - ln
        pleft = int(np.fix(dlt / 2)) + int(np.fmod(dlt, 2))
        for c in range(cell):
            sc = c - pleft
            if 0 <= sc < ln:
                px[:, margin + j * cell + c] = strip[:, start + sc]
        start += ln
    return px.astype(np.float32) / np.float32(255)


def model_batch(bases, plan, T_src, T_mel, cell, margin, W_out=None):
    """What ``vo_augment_batch`` writes for ``plan`` (rows of 5 ints, any values) -> dict of numpy arrays with the
    dtypes of ``to_device``'s batch, + status."""
    B, U = len(plan), len(bases)
    n_mels, H = bases[0]["mel"].shape[1], bases[0]["image"][0].shape[0]
    W_out = T_src * cell + 2 * margin if W_out is None else W_out
    o = {"audiotypes": np.zeros(B, np.int64), "texts": np.zeros((B, T_src), np.int64), "src_lens": np.zeros(B, np.int64),
         "mels": np.zeros((B, T_mel, n_mels), np.float32), "mel_lens": np.zeros(B, np.float32),
         "energies": np.zeros((B, T_src), np.float32), "kurtosises": np.zeros((B, T_src), np.float32),
         "durations": np.zeros((B, T_src), np.float32), "images": np.ones((B, 1, H, W_out), np.float32),
         "status": np.zeros(B, np.int32)}
    for b, (src, pos, m, mm, r) in enumerate(np.asarray(plan).tolist()):
        if not (0 <= src < U and m >= 0 and mm >= 0 and r >= 1 and 0 <= pos < len(bases[src]["text"])):
            o["status"][b] = BAD_ROW
            continue
        u = bases[src]
        if (len(u["text"]) + m) * r > T_src:
            o["status"][b] = CHARS_OVER
            continue
        if (int(u["duration"].sum()) + mm * int(u["duration"][pos])) * r > T_mel:
            o["status"][b] = FRAMES_OVER
            continue
        v = model_row(u, pos, m, mm, r)
        L, FL = len(v["text"]), v["mel"].shape[0]
        o["audiotypes"][b], o["src_lens"][b], o["mel_lens"][b] = v["audiotype"], L, FL
        o["texts"][b, :L], o["mels"][b, :FL], o["durations"][b, :L] = v["text"], v["mel"], v["duration"]
        o["energies"][b, :L], o["kurtosises"][b, :L] = v["energy"], v["kurtosis"]  # float64 -> float32 as .float()
        o["images"][b, 0] = layout(v["image"][0], v["image"][1], cell, margin, W_out)
    return o


def plan_of(variant_name, base, mel_copies="reference"):
    """(pos, m, m_mel, r) of a golden variant, by its name among ``variants()`` of its base."""
    from visual_onoma_to_wave_amd.preprocessor import augment as AU
    cfg = load()["cfg_b"]
    for suffix, pos, m, mm, r, _ in AU.variants(base["text_str"], cfg, mel_copies):
        if base["id"] + suffix == variant_name:
            return pos, m, mm, r
    raise KeyError(variant_name)
