"""Repeat / consecutive augmentation, host side: which variants exist, the index maps as a
numpy model, plan and pack-time validation -- against the files the reference's own ``_augmentation`` wrote
(tests/golden/augment.npz, make_goldens_augment.py).  Every comparison is exact."""

import copy
import os

import numpy as np
import pytest

import augment_check as C
from visual_onoma_to_wave_amd.preprocessor import augment as AU


@pytest.fixture(scope="module")
def g():
    return C.load()


def test_consecutive_pos_equals_the_reference(g):
    assert len(g["cpos"]) >= 40
    assert {p for _, p in g["cpos"]} >= {None, 1, 2, 3, 6}  # a run's middle is never position 0
    for text, pos in g["cpos"]:
        assert AU.consecutive_pos(text) == pos, text
        assert AU.consecutive_pos([ord(c) for c in text]) == pos, text  # ids as well as strings


@pytest.mark.parametrize("which", ["a", "b"])
def test_variants_names_order_and_texts(g, which):
    cfg, order = g["cfg_" + which], g["order_" + which]
    assert cfg["first_consecutive"] == (0 if which == "a" else 2)
    names, texts = [], []
    for u in g["bases"]:
        for suffix, pos, m, m_mel, r, text in AU.variants(u["text_str"], cfg):
            assert AU.is_variant_name(u["id"] + suffix) and r >= 1 and m_mel == (m + 1 if m else 0)
            assert len(text) == (len(u["text_str"]) + m) * r
            names.append(u["id"] + suffix)
            texts.append(text)
    assert names == [g["variants"][i]["id"] for i in order]
    assert texts == [g["variants"][i]["text_str"] for i in order]
    assert not any(AU.is_variant_name(u["id"]) for u in g["bases"])
    # the golden has what it was made for: a text over max_length without variants, nested repeats cut off by
    # the augmented text's length, a run at the end of a text
    per_base = [sum(1 for n in names if n.startswith(u["id"])) for u in g["bases"]]
    assert 0 in per_base and len(set(per_base)) >= 4


def test_variants_of_symbol_ids(g):
    u = g["bases"][3]
    by_str = AU.variants(u["text_str"], g["cfg_b"])
    by_ids = AU.variants(u["text"], g["cfg_b"])
    assert [v[:5] for v in by_str] == [v[:5] for v in by_ids]
    sym = C.symbol_ids()
    assert [[sym[c] for c in v[5]] for v in by_str] == [list(v[5]) for v in by_ids]


def test_model_reproduces_every_reference_file(g):
    """The index maps with mel_copies="reference" give every array of every variant the reference wrote: text, the
    per-character arrays with their dtypes, the mel (one copy of the character's frames more than the durations
    say), the strip and its widths."""
    assert len(g["variants"]) >= 50
    zero_dur = 0
    for v in g["variants"]:
        u = g["bases"][v["src"]]
        pos, m, m_mel, r = C.plan_of(v["id"], u)
        w = C.model_row(u, pos, m, m_mel, r)
        for k in ("text", "mel", "energy", "kurtosis", "duration"):
            assert w[k].dtype == v[k].dtype and np.array_equal(w[k], v[k]), (v["id"], k)
        assert np.array_equal(w["image"][0], v["image"][0]) and np.array_equal(w["image"][1], v["image"][1]), v["id"]
        assert v["mel"].shape[0] == (u["mel"].shape[0] + m_mel * int(u["duration"][pos])) * r
        if m:
            assert v["mel"].shape[0] == int(v["duration"].sum()) + r * int(u["duration"][pos])
            zero_dur += int(u["duration"][pos]) == 0
    assert zero_dur >= 5  # the zero-duration character was augmented


def test_durations_mode_matches_the_durations(g):
    n = 0
    for u in g["bases"]:
        for suffix, pos, m, m_mel, r, _ in AU.variants(u["text_str"], g["cfg_b"], mel_copies="durations"):
            assert m_mel == m
            w = C.model_row(u, pos, m, m_mel, r)
            assert w["mel"].shape[0] == int(w["duration"].sum())
            n += 1
    assert n == len(g["order_b"])
    with pytest.raises(ValueError, match="mel_copies"):
        AU.variants("アアア", g["cfg_a"], mel_copies="both")


def _corpus(g, utterances=None):
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    return DeviceCorpus.from_arrays(g["bases"] if utterances is None else utterances, 102, 1, "cpu")


@pytest.mark.parametrize("row, caps, rule", [
    ((7, 0, 0, 0, 1), (None, None), r"src is outside \[0, 7\)"),
    ((-1, 0, 0, 0, 1), (None, None), "src is outside"),
    ((0, 2, 0, 0, 1), (None, None), r"pos is outside \[0, 2\)"),
    ((0, -1, 0, 0, 1), (None, None), "pos is outside"),
    ((0, 0, -1, 0, 1), (None, None), "m and m_mel must be >= 0 and r >= 1"),
    ((0, 0, 0, -1, 1), (None, None), "m and m_mel must be >= 0 and r >= 1"),
    ((0, 0, 0, 0, 0), (None, None), "m and m_mel must be >= 0 and r >= 1"),
    ((0, 1, 2, 3, 2), (7, 1000), "8 characters are over max_src_len = 7"),
    ((0, 0, 0, 0, 2), (8, 4), "8 frames are over max_mel_len = 4"),  # base 0 has 4 frames
])
def test_host_plan_is_checked_before_anything_is_launched(g, row, caps, rule):
    """A corpus on the CPU cannot launch: the ValueError is raised by the host check, and names row 1."""
    corpus = _corpus(g)
    with pytest.raises(ValueError, match=r"plan row 1 \(src .*" + rule):
        corpus.batch([(0, 0, 0, 0, 1), row], *caps)
    assert corpus.last_status is None
    with pytest.raises(ValueError, match=r"shape \(B, 5\)"):
        corpus.batch(np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="integers"):
        corpus.batch(np.zeros((2, 5), np.float32))


def test_check_plan_sizes(g):
    corpus = _corpus(g)
    u = g["bases"][4]  # the zero duration at its run's middle
    pos = AU.consecutive_pos(u["text_str"])
    assert int(u["duration"][pos]) == 0
    plan, src_lens, mel_lens = AU.check_plan([(4, pos, 2, 3, 2), (0, 1, 1, 2, 3)], corpus.n_chars, corpus.n_frames,
                                             corpus.durations)
    assert plan.dtype == np.int32 and plan.shape == (2, 5)
    d0 = g["bases"][0]["duration"]
    assert src_lens == [(5 + 2) * 2, (2 + 1) * 3]
    assert mel_lens == [int(u["duration"].sum()) * 2, (int(d0.sum()) + 2 * int(d0[1])) * 3]


def test_corpus_variants_rows(g):
    corpus = _corpus(g)
    names, plan = corpus.variants(g["cfg_a"])
    assert plan.dtype == np.int32 and plan.shape == (len(g["bases"]) + len(g["order_a"]), 5)
    assert [n for n in names if AU.is_variant_name(n)] == [g["variants"][i]["id"] for i in g["order_a"]]
    assert [n for n in names if not AU.is_variant_name(n)] == [u["id"] for u in g["bases"]]
    for name, (src, pos, m, m_mel, r) in zip(names, plan.tolist()):
        assert name == g["bases"][src]["id"] + AU.suffix_of(g["bases"][src]["text"], pos, m, r)


@pytest.mark.parametrize("edit, message", [
    (lambda u: u.update(mel=u["mel"][:-1]), "the durations sum to"),
    (lambda u: u.update(image=(u["image"][0][:, :-1], u["image"][1])), "the widths sum to"),
    (lambda u: u.update(energy=u["energy"][:-1]), "the text has 4 characters"),
    (lambda u: u.update(duration=np.append(u["duration"], 0)), "the text has 4 characters"),
    (lambda u: u.update(image=(u["image"][0], u["image"][1][:-1])), "the text has 4 characters"),
    (lambda u: u.update(kurtosis=None), "kurtosis is given for some"),
])
def test_pack_time_checks_name_the_utterance(g, edit, message):
    us = [copy.copy(u) for u in g["bases"]]
    edit(us[2])
    with pytest.raises(ValueError, match=r"utterance 2 \('ipaexg_24pt_maracas-a1-003'\).*" + message):
        _corpus(g, us)


def test_is_variant_name():
    base = "ipaexg_24pt_drum-a1-001"
    for suffix in ("-repeat2", "-repeat13", "-firstconsecutive1", "-consecutive5", "-consecutive1-repeat3",
                   "-firstconsecutive2-repeat2"):
        assert AU.is_variant_name(base + suffix), suffix
    for name in (base, base + "-repeat", base + "-consecutive", "repeat2-" + base, base + "-repeat2-x"):
        assert not AU.is_variant_name(name), name


def test_from_dataset_keeps_the_base_utterances(g, tmp_path):
    """A preprocessed directory whose metadata already lists variants, read through ``Dataset``: ``from_dataset`` packs
    the base utterances only (each through ``ds[i]``), or everything it is pointed at with ``base_only=False``."""
    import shutil
    from PIL import Image
    from helpers import DATA, configs, golden
    from visual_onoma_to_wave_amd.dataset import Dataset, DeviceCorpus
    labels = [str(x) for x in golden("augment")["base_labels"]]
    items = [(u, labels[i]) for i, u in enumerate(g["bases"][:3])]
    items += [(v, labels[v["src"]]) for v in g["variants"] if v["src"] < 3][:5]
    for f in ("visual_text.json", "audiotype.json", "symbols.json"):
        shutil.copy(os.path.join(DATA, f), tmp_path / f)
    lines = []
    for u, label in items:
        for sub, a in (("mel", u["mel"]), ("energy", u["energy"]), ("kurtosis", u["kurtosis"]),
                       ("duration", u["duration"]), ("image/width", u["image"][1])):
            (tmp_path / sub / label).mkdir(parents=True, exist_ok=True)
            np.save(tmp_path / sub / label / f"{u['id']}.npy", a)
        (tmp_path / "image/png" / label).mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.repeat(u["image"][0][:, :, None], 3, axis=2)).save(
            tmp_path / "image/png" / label / f"{u['id']}.png")
        lines.append(f"{u['id']}|{label}|24|ipaexg|{u['text_str']}")
    (tmp_path / "train.txt").write_text("\n".join(lines[3:] + lines[:3]) + "\n", encoding="utf-8")  # variants first
    pc, mc, tc = configs()
    pc = dict(pc, path=dict(pc["path"], preprocessed=str(tmp_path)))
    ds = Dataset("train.txt", pc, tc, mc)
    corpus = DeviceCorpus.from_dataset(ds, device="cpu")
    assert corpus.names == [u["id"] for u in g["bases"][:3]] and len(corpus) == 3
    assert (corpus.cell, corpus.stride, corpus.height, corpus.n_mels) == (102, 1, 24, 80)
    assert corpus.texts == [tuple(u["text"].tolist()) for u in g["bases"][:3]]
    assert corpus.n_frames == [u["mel"].shape[0] for u in g["bases"][:3]]
    assert corpus.tensors["ch_kurtosis"] is None and corpus.tensors["ch_energy"] is not None  # as the model config
    assert np.array_equal(corpus.tensors["mel"].numpy(), np.concatenate([u["mel"] for u in g["bases"][:3]]))
    assert len(DeviceCorpus.from_dataset(ds, base_only=False, device="cpu")) == 8
    assert DeviceCorpus.from_dataset(ds, indices=[6, 0], device="cpu").names == [g["bases"][1]["id"]]
