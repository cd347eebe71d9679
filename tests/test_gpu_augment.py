"""Repeat / consecutive augmentation on the GPU (vo_augment_batch, dataset.DeviceCorpus).
Every output is a copy: every comparison is ``torch.equal``, dtype for dtype.  The base corpus is the golden's
(tests/golden/augment.npz: seven utterances of 1 to 8 characters, at most 40 frames); the numpy model of the index
maps is tests/augment_check.py, which tests/test_augment_cpu.py holds against the reference's own files."""

import numpy as np
import pytest
import torch

import augment_check as C
from helpers import configs, vtts_arrays
from weights import load_into

pytestmark = pytest.mark.gpu

KEYS = ("audiotypes", "texts", "src_lens", "mels", "mel_lens", "energies", "kurtosises", "durations", "images")
IDX = dict(zip(KEYS, (1, 2, 3, 5, 6, 8, 9, 10, 11)))  # their places in the 13-item batch tuple

# base utterances: 0 "ワン" (4 frames), 1 one character, 2 a run at the end (n = 4), 3 a run in the middle (n = 5),
# 4 a zero duration at position 2 (n = 5), 5 seven characters, 6 eight characters
ROWS = [
    (0, 0, 0, 0, 1),                                                             # the identity
    (1, 0, 0, 0, 3),                                                             # n = 1, r = 3
    (2, 0, 1, 2, 1), (2, 0, 2, 2, 1), (2, 0, 3, 4, 1), (2, 0, 4, 4, 1), (2, 0, 5, 6, 1),   # pos = 0, m = 1 .. 5
    (2, 3, 1, 1, 1), (2, 3, 2, 3, 1), (2, 3, 3, 3, 1), (2, 3, 4, 5, 1), (2, 3, 5, 5, 1),   # pos = n - 1, m_mel = m, m + 1
    (4, 2, 2, 3, 1), (4, 2, 4, 4, 2),                                            # d[pos] = 0
    (0, 1, 2, 3, 3), (3, 2, 2, 2, 3),                                            # r = 3 on top of m = 2
    (5, 6, 1, 2, 1), (5, 0, 0, 0, 2), (6, 7, 1, 1, 1), (6, 0, 0, 0, 1), (3, 4, 0, 3, 1),   # long rows; m_mel without m
]
BATCHES = [ROWS[0:7], ROWS[7:14], ROWS[14:21], [ROWS[14]], [ROWS[1]]]  # B = 7 (the same src in several rows) and B = 1


@pytest.fixture(scope="module")
def g():
    return C.load()


@pytest.fixture(scope="module")
def corpora(g, device):
    """DeviceCorpus and the bases it was packed from, by (cell, stride, n_mels); packed once each."""
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    made = {}

    def get(cell, stride, n_mels=80, kurtosis=True):
        key = (cell, stride, n_mels, kurtosis)
        if key not in made:
            bases = [dict(u, mel=np.ascontiguousarray(u["mel"][:, :n_mels]), kurtosis=u["kurtosis"] if kurtosis else None)
                     for u in g["bases"]]
            made[key] = (DeviceCorpus.from_arrays(bases, cell, stride, device), bases)
        return made[key]
    return get


def _caps(bases, plan, extra=0):
    sizes = [((len(bases[s]["text"]) + m) * r, (int(bases[s]["duration"].sum()) + mm * int(bases[s]["duration"][p])) * r)
             for s, p, m, mm, r in plan]
    return max(a for a, _ in sizes) + extra, max(b for _, b in sizes) + 3 * extra


def _assert_equal(got, want, what=""):
    """``got``: name -> tensor; ``want``: the numpy model's dict."""
    for k in KEYS + (("status",) if "status" in got else ()):
        w = torch.from_numpy(want[k])
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k, got[k].dtype, tuple(got[k].shape))
        assert torch.equal(got[k].cpu(), w), (what, k)


def _named(batch, status=None):
    d = {k: batch[i] for k, i in IDX.items()}
    if status is not None:
        d["status"] = status
    return d


@pytest.mark.parametrize("cell, stride, n_mels", [
    (102, 1, 80),   # the packaged geometry: no margin, 16-byte frames
    (102, 3, 80),   # a margin
    (24, 3, 5),     # characters wider than the cell (widths 5 .. 40), the scalar mel path
    (24, 1, 80),
])
@pytest.mark.parametrize("extra", [0, 2])  # caps exactly the longest row, and larger
def test_case_matrix(corpora, device, cell, stride, n_mels, extra):
    corpus, bases = corpora(cell, stride, n_mels)
    assert max(int(u["image"][1].max()) for u in bases) > 24 >= min(int(u["image"][1].min()) for u in bases)
    for plan in BATCHES:
        T_src, T_mel = _caps(bases, plan, extra)
        plan_d = torch.tensor(plan, dtype=torch.int32, device=device)
        batch = corpus.batch(plan_d, T_src, T_mel)
        want = C.model_batch(bases, plan, T_src, T_mel, cell, corpus.margin)
        assert batch[0] is None and batch[4] == T_src and batch[7] == T_mel and batch[12] is None
        assert want["status"].tolist() == [0] * len(plan)
        _assert_equal(_named(batch, corpus.last_status), want, (plan, T_src, T_mel))
        assert batch[11].shape == (len(plan), 1, 24, T_src * cell + 2 * (stride // 2) * cell)


@pytest.mark.parametrize("cell, stride, n_mels", [(102, 3, 80), (24, 1, 5)])
def test_wider_image_through_the_op(corpora, device, cell, stride, n_mels):
    """``ops.augment_batch`` itself, with a W_out wider than the caps need (odd: rows that are not 16-byte aligned)."""
    from visual_onoma_to_wave_amd import ops
    corpus, bases = corpora(cell, stride, n_mels)
    plan = BATCHES[2]
    T_src, T_mel = _caps(bases, plan, 1)
    W_out = T_src * cell + 2 * corpus.margin + 37
    got = ops.augment_batch(corpus.struct, torch.tensor(plan, dtype=torch.int32, device=device), T_src, T_mel, 24, cell,
                            corpus.margin, W_out=W_out)
    _assert_equal(got, C.model_batch(bases, plan, T_src, T_mel, cell, corpus.margin, W_out))
    with pytest.raises(ValueError, match="W_out"):
        ops.augment_batch(corpus.struct, torch.tensor(plan, dtype=torch.int32, device=device), T_src, T_mel, 24, cell,
                          corpus.margin, W_out=T_src * cell + 2 * corpus.margin - 1)
    with pytest.raises(RuntimeError, match="strip height"):
        ops.augment_batch(corpus.struct, torch.tensor(plan, dtype=torch.int32, device=device), T_src, T_mel, 25, cell,
                          corpus.margin)


def test_equals_the_host_path_on_the_reference_files(g, corpora, device):
    """Every file the reference's ``_augmentation`` wrote, read as ``Dataset.__getitem__`` reads it, through
    ``Dataset.reprocess`` (pad_1D / pad_2D / GlyphBatch) and ``to_device``, against ``corpus.batch`` of the plan rows
    ``corpus.variants`` gives for the same names: ids, sizes, and every tensor element for element, dtype for dtype."""
    from visual_onoma_to_wave_amd.dataset import Dataset
    from visual_onoma_to_wave_amd.utils.tools import to_device
    corpus, bases = corpora(102, 1)
    ds = object.__new__(Dataset)  # reprocess reads these three only
    ds.use_image, ds.width, ds.stride = True, corpus.cell, corpus.stride
    names, plan = corpus.variants(g["cfg_b"])
    items = {v["id"]: v for v in g["variants"] + g["bases"]}
    assert sorted(names) == sorted(items) and len(names) == 60
    for lo in range(0, len(names), 16):
        rows = slice(lo, lo + 16)
        data = [items[n] for n in names[rows]]
        want = to_device(ds.reprocess(data, list(range(len(data)))), device)
        got = corpus.batch(plan[rows])
        assert got[0] == want[0] == names[rows]
        assert (got[4], got[7]) == (int(want[4]), int(want[7])) and got[12] is None and want[12] is None
        for k, i in IDX.items():
            assert got[i].dtype == want[i].dtype and got[i].shape == want[i].shape, (lo, k)
            assert torch.equal(got[i], want[i]), (lo, k)
        assert corpus.last_status.tolist() == [0] * len(data)


def test_refused_rows_come_out_empty_and_nothing_is_left_unwritten(corpora, device):
    corpus, bases = corpora(102, 3)
    good = [(0, 1, 2, 3, 3), (3, 2, 1, 2, 1), (5, 6, 0, 0, 1)]
    T_src, T_mel = _caps(bases, good)
    F6 = int(bases[6]["duration"].sum())
    assert F6 * 2 > T_mel and (8 + 1) <= T_src < 8 * 2
    plan = [good[0],
            (7, 0, 0, 0, 1), (-1, 0, 0, 0, 1),                    # src
            good[1],
            (2, 4, 0, 0, 1), (2, -1, 0, 0, 1),                    # pos
            (0, 0, 0, 0, 0), (0, 0, -1, 0, 1), (0, 0, 0, -2, 1),  # r, m, m_mel
            (6, 0, 0, 0, 2), (6, 0, T_src, 0, 1),                 # characters over the cap
            (4, 0, 0, T_mel, 1), (3, 0, 0, 3, 2),                 # frames over the cap: F' alone, and F' r
            (0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),        # products that would overflow 32 bits
            good[2]]
    status = [0, 1, 1, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3, 2, 0]
    assert int(bases[4]["duration"][0]) * T_mel + int(bases[4]["duration"].sum()) > T_mel
    d3 = bases[3]["duration"]
    assert int(d3.sum()) + 3 * int(d3[0]) <= T_mel < 2 * (int(d3.sum()) + 3 * int(d3[0])) and 5 * 2 <= T_src
    plan_d = torch.tensor(plan, dtype=torch.int32, device=device)
    out = corpus.batch(plan_d, T_src, T_mel)
    for i in IDX.values():  # a sentinel in every element of every output
        out[i].fill_(float("nan") if out[i].is_floating_point() else -7)
    corpus.last_status.fill_(-7)
    st = corpus.last_status
    again = corpus.batch(plan_d, T_src, T_mel, out=out)
    assert all(again[i].data_ptr() == out[i].data_ptr() for i in IDX.values()) and corpus.last_status is st
    want = C.model_batch(bases, plan, T_src, T_mel, 102, corpus.margin)
    assert want["status"].tolist() == status
    _assert_equal(_named(again, corpus.last_status), want)
    refused = [b for b, s in enumerate(status) if s]
    for k, pad in (("texts", 0), ("mels", 0), ("durations", 0), ("energies", 0), ("kurtosises", 0), ("src_lens", 0),
                   ("mel_lens", 0), ("images", 1)):
        assert bool((again[IDX[k]][refused] == pad).all()), k


def test_host_plan_refusal_launches_nothing(corpora, device):
    corpus, _ = corpora(102, 1)
    before = corpus.last_status
    with pytest.raises(ValueError, match=r"plan row 1 .*pos is outside"):
        corpus.batch([(0, 0, 0, 0, 1), (0, 2, 0, 0, 1)])
    with pytest.raises(ValueError, match="needs max_src_len and max_mel_len"):
        corpus.batch(torch.zeros((1, 5), dtype=torch.int32, device=device))
    assert corpus.last_status is before


def test_graph_replay_follows_a_plan_rewritten_in_place(corpora, device):
    import visual_onoma_to_wave_amd  # noqa: F401  (before the first GPU call: its import-time runtime setting)
    corpus, bases = corpora(102, 1)
    first, second = BATCHES[0], BATCHES[2]
    T_src, T_mel = (max(a, b) for a, b in zip(_caps(bases, first), _caps(bases, second)))
    plan_d = torch.tensor(first, dtype=torch.int32, device=device)
    static = corpus.batch(plan_d, T_src, T_mel)  # warm outside the capture; the static batch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        corpus.batch(plan_d, T_src, T_mel, out=static)
    status = corpus.last_status
    for plan in (second, first):
        plan_d.copy_(torch.tensor(plan, dtype=torch.int32, device=device))
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_named(static, status), C.model_batch(bases, plan, T_src, T_mel, 102, 0), plan)


def test_train_step_takes_the_device_batch(g, corpora, device):
    """One step of the packaged test model on a device-assembled batch of mixed variants (without kurtosis, as a
    Dataset of this model configuration gives it; the mel of the durations, which is what the length regulator
    makes)."""
    from visual_onoma_to_wave_amd.model import FastSpeech2Loss, ScheduledOptim, vTTS
    from visual_onoma_to_wave_amd.train import train_step
    pc, mc, tc = configs()
    assert not mc["variance_embedding"]["is_kurtosis_condition"] and pc["visual_text"]["stride"] == 1
    corpus, _ = corpora(102, 1, kurtosis=False)
    names, plan = corpus.variants(g["cfg_a"], mel_copies="durations")
    pick = [i for i, n in enumerate(names) if n.endswith(("-003", "-consecutive2", "-repeat2", "-consecutive1-repeat3"))]
    batch = corpus.batch(plan[pick])
    assert len(pick) >= 8 and batch[9] is None and batch[8] is not None
    assert torch.equal(batch[10].sum(1), batch[6])  # the durations sum to the mel lengths
    m = vTTS(pc, mc, tc)
    load_into(m, vtts_arrays())
    m = m.to(device).train()
    losses = train_step(m, ScheduledOptim(m, tc, mc, 0), FastSpeech2Loss(), batch)
    assert all(bool(torch.isfinite(torch.as_tensor(x)).all()) for x in losses)
    assert float(losses[0].detach()) > 0
