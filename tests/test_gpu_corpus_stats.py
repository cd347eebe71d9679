"""Corpus statistics over the augmented population on the GPU (vo_corpus_stats, vo_corpus_normalize,
``DeviceCorpus.stats`` / ``normalize_``) against the numpy float64 model of
tests/corpus_stats_check.py, which tests/test_corpus_stats_cpu.py holds against the reference's own
``_remove_outlier`` and ``StandardScaler``.

Kept counts, raw min / max and statuses are exact.  Mean and std are held to a derived bar: for N kept values
|mean - ref| <= N 2^-52 (|ref mean| + ref std) and |std - ref| <= N 2^-52 ref std, the worst case of a plain float64
summation of N terms, whatever the order of combining them.  Each test prints its worst ratio to that bar."""

import numpy as np
import pytest
import torch

import augment_check as C
import corpus_stats_check as S

pytestmark = pytest.mark.gpu

# characters of the synthetic base utterances; their values are seeded float32 draws unless named below
SIZES = [1, 4, 2, 3, 4, 5, 21, 30, 11, 125, 40, 64, 8]
EQUAL, COINCIDE = 1, 12   # all values equal; [5, 0, 5, 5, 5, 9, 5, 5]: the quartiles coincide, 0 and 9 are outliers
MAXR = S.MAX_CHARS // 64  # utterance 11 (64 characters) repeated MAXR times is VO_STATS_MAX_CHARS characters

EDGES = (
    [(u, 0, 0, 0, 1) for u in range(len(SIZES))]                          # identity rows: L = 1 .. 5 among them
    + [(6, 3, 0, 0, 3), (7, 29, 2, 3, 2), (8, 5, 2, 2, 5)]                # L = 63, 64, 65
    + [(9, 60, 2, 3, 1), (7, 0, 2, 2, 4), (10, 39, 3, 4, 3)]              # L = 127, 128, 129
    + [(5, 0, m, m + 1, 1) for m in range(1, 6)]                          # pos = 0, m = 1 .. 5
    + [(5, 4, m, m, 1) for m in range(1, 6)]                              # pos = n - 1
    + [(5, 2, 2, 3, 3), (3, 1, 2, 2, 3)]                                  # r = 3 on m = 2
    + [(3, 1, 8, 8, 1)]                                                   # [a, b x 9, c]: quartiles coincide at b
    + [(0, 0, 0, 0, 3), (0, 0, 4, 0, 1)]                                  # n = 1 repeated and stretched: all equal
    + [(13, 0, 0, 0, 1), (2, 2, 0, 0, 1), (2, 0, -1, 0, 1), (2, 0, 0, -1, 1), (2, 0, 0, 0, 0)]   # bad rows ...
    + [(4, 1, 1, 9, 2)]                                                   # ... in the middle of good ones
)
STATUS_EDGES = [0] * 34 + [1] * 5 + [0]
AT_CAP = [(11, 0, 0, 0, MAXR), (11, 0, 1, 1, MAXR), (11, 0, 0, 0, MAXR + 1), (11, 63, 0, 0, 1),
          (11, 0, 2 ** 31 - 1, 0, 2 ** 31 - 1)]                           # products that would overflow 32 bits
STATUS_AT_CAP = [0, 4, 4, 0, 4]


def _plan300():
    """300 rows cycling over the utterances with every kind of variant: the combine tree has odd levels (256 + 44
    strided partials) and rows that keep nothing in between."""
    rng = np.random.default_rng(300)
    rows = []
    for i in range(300):
        u = int(rng.integers(0, 11))
        rows.append((u, int(rng.integers(0, SIZES[u])), int(rng.integers(0, 4)), int(rng.integers(0, 4)),
                     int(rng.integers(1, 4))))
    return rows


PLANS = {"edges": EDGES, "at_cap": AT_CAP, "rows300": _plan300(), "one_row": [EDGES[9]], "one_row_n1": [EDGES[0]],
         "one_row_at_cap": [AT_CAP[0]], "one_row_refused": [AT_CAP[1]]}
worst = {"mean": 0.0, "std": 0.0}


@pytest.fixture(scope="module")
def synth(device):
    """(DeviceCorpus, {feature: list of float32 arrays}): 13 utterances of one frame and one pixel column a
    character (the statistics read neither)."""
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    rng = np.random.default_rng(15)
    values = {f: [(rng.standard_normal(n) * (1.0 if f == "energy" else 3.0) + (0.3 if f == "energy" else -2.0))
                  .astype(np.float32) for n in SIZES] for f in S.FEATURES}
    for f in S.FEATURES:
        values[f][EQUAL][:] = values[f][EQUAL][0]
        values[f][COINCIDE][:] = [5, 0, 5, 5, 5, 9, 5, 5]
    utts = [{"id": f"u{i}", "audiotype": i % 3, "text": np.arange(1, n + 1), "mel": np.zeros((n, 4), np.float32),
             "energy": values["energy"][i], "kurtosis": values["kurtosis"][i], "duration": np.ones(n, np.int64),
             "image": (np.zeros((2, n), np.uint8), np.ones(n, np.int32)), "event_image_feature": None}
            for i, n in enumerate(SIZES)]
    return DeviceCorpus.from_arrays(utts, 4, 1, device), values


def _check(out, status, want, what):
    """Device ``out`` (6 float64 on the host) and status against the model's dict."""
    assert want["margin"] > 1e-9, (what, want["margin"])  # the kept count is well defined
    assert status.tolist() == want["status"].tolist(), what
    assert out[0] == want["count"] and out[5] == want["rows_used"], (what, out, want["count"], want["rows_used"])
    assert out[3] == want["raw_min"] and out[4] == want["raw_max"], (what, out)
    bm, bs = S.bar(want)
    rm, rs = abs(out[1] - want["mean"]) / bm, abs(out[2] - want["std"]) / bs
    worst["mean"], worst["std"] = max(worst["mean"], rm), max(worst["std"], rs)
    print(f"corpus_stats {what}: N {want['count']}, ratio to the bar: mean {rm:.4f}, std {rs:.4f} "
          f"(worst so far {worst['mean']:.4f}, {worst['std']:.4f})")
    assert rm <= 1 and rs <= 1, (what, out, want["mean"], want["std"])


@pytest.mark.parametrize("feature", S.FEATURES)
@pytest.mark.parametrize("name", list(PLANS))
def test_device_against_the_model(synth, device, name, feature):
    from visual_onoma_to_wave_amd import ops
    corpus, values = synth
    plan = PLANS[name]
    want = S.model(values[feature], plan)
    if name == "edges":
        assert want["status"].tolist() == STATUS_EDGES
        lens = [(SIZES[s] + m) * r for s, _, m, _, r in plan[:34]]
        assert set(lens) >= {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129}
        assert len(want["kept"][COINCIDE]) == 0 and len(want["kept"][EQUAL]) == 0 and len(want["kept"][0]) == 0
        assert len(want["kept"][31]) == 0 and len(np.unique(S.row_array(values[feature][3], plan[31]))) == 3
    if name == "at_cap":
        assert want["status"].tolist() == STATUS_AT_CAP and (SIZES[11] * MAXR, SIZES[11] + 1) == (S.MAX_CHARS, 65)
    out, status = ops.corpus_stats(corpus.struct, torch.tensor(plan, dtype=torch.int32, device=device), feature)
    _check(out.cpu().numpy(), status.cpu().numpy(), want, f"{name} {feature}")


def test_corpus_stats_method_and_refusals(synth, device):
    """``DeviceCorpus.stats``: the ``stats.json`` layout from a host plan, the base rows by default, a host plan
    checked before anything is launched, a device plan taken unread."""
    from visual_onoma_to_wave_amd import _lib, ops
    corpus, values = synth
    got = corpus.stats(EDGES[:34])
    assert list(got) == ["energy", "kurtosis"] and corpus.last_status.tolist() == [0] * 34
    for f in S.FEATURES:
        want = S.model(values[f], EDGES[:34])
        js = S.stats_json(want)
        bm, bs = S.bar(want)
        assert abs(got[f][2] - js[2]) <= bm and abs(got[f][3] - js[3]) <= bs
        mean, std = np.float64(got[f][2]), np.float64(got[f][3])  # min / max: exact, given the device's mean and std
        assert got[f][0] == float((np.float64(want["raw_min"]) - mean) / std)
        assert got[f][1] == float((np.float64(want["raw_max"]) - mean) / std)
    base = corpus.stats()
    assert base["energy"][2:] == corpus.stats([(u, 0, 0, 0, 1) for u in range(len(SIZES))])["energy"][2:]
    before = corpus.last_status
    with pytest.raises(ValueError, match=r"plan row 1 .*pos is outside"):
        corpus.stats([(0, 0, 0, 0, 1), (0, 1, 0, 0, 1)])
    assert corpus.last_status is before
    over = corpus.stats(torch.tensor(AT_CAP, dtype=torch.int32, device=device))  # a device plan: refused on the device
    assert corpus.last_status.tolist() == STATUS_AT_CAP and over["energy"][3] > 0
    assert corpus.stats(AT_CAP) == over and corpus.last_status.tolist() == STATUS_AT_CAP  # a host plan has no cap either
    with pytest.raises(ValueError, match="no plan row was accepted"):
        corpus.stats([AT_CAP[1]])
    with pytest.raises(ValueError, match="feature must be one of"):
        ops.corpus_stats(corpus.struct, torch.zeros((1, 5), dtype=torch.int32, device=device), "mel")
    with pytest.raises(ValueError, match="workspace must be uint8"):
        ops.corpus_stats(corpus.struct, torch.zeros((3, 5), dtype=torch.int32, device=device), "energy",
                         workspace=torch.empty(3 * 40 - 1, dtype=torch.uint8, device=device))
    no_k = _lib.Corpus.from_buffer_copy(corpus.struct)
    no_k.ch_kurtosis = None
    with pytest.raises(ValueError, match="packed without kurtosis"):
        ops.corpus_stats(no_k, torch.zeros((1, 5), dtype=torch.int32, device=device), "kurtosis")
    plan_d, ws, out = (torch.zeros(n, dtype=dt, device=device) for n, dt in ((5, torch.int32), (40, torch.uint8),
                                                                             (6, torch.float64)))
    rc = _lib.lib().vo_corpus_stats(no_k, plan_d.data_ptr(), 1, _lib.STATS_KURTOSIS, ws.data_ptr(), 40, out.data_ptr(),
                                    None, None)  # the entry itself refuses too
    assert rc == -1 and b"without kurtosis" in _lib.lib().vo_last_error()


def test_two_calls_give_the_same_bits(synth, device):
    from visual_onoma_to_wave_amd import ops
    corpus, _ = synth
    plan = torch.tensor(PLANS["rows300"] + EDGES + AT_CAP, dtype=torch.int32, device=device)
    for f in S.FEATURES:
        a, sa = ops.corpus_stats(corpus.struct, plan, f)
        b, sb = ops.corpus_stats(corpus.struct, plan, f)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert torch.equal(sa, sb)


@pytest.fixture(scope="module")
def golden_corpus(device):
    from visual_onoma_to_wave_amd.dataset import DeviceCorpus
    g = C.load()
    return g, (lambda: DeviceCorpus.from_arrays(g["bases"], 102, 1, device))


@pytest.mark.parametrize("feature", S.FEATURES)
def test_golden_files_as_a_plan(golden_corpus, device, feature):
    """The 60 files of the golden as plan rows over its 7 base utterances: the kept count is the reference's, mean
    and std are ``StandardScaler``'s over what the reference's ``_remove_outlier`` kept of the files as the corpus
    holds them (float32)."""
    from visual_onoma_to_wave_amd import ops
    g, make = golden_corpus
    gs = S.load()
    names, plan = S.golden_plan(g)
    kept = gs[f"{feature}_f32_kept"]
    mean, scale = gs[f"{feature}_f32_scaler"]
    values = [u[feature].astype(np.float32) for u in g["bases"]]
    want = dict(S.model(values, plan), mean=mean, std=scale)
    assert want["count"] == sum(len(k) for k in kept) and want["rows_used"] == sum(len(k) > 0 for k in kept)
    corpus = make()  # alive while the kernels read it: the struct holds addresses only
    out, status = ops.corpus_stats(corpus.struct, torch.from_numpy(plan).to(device), feature)
    _check(out.cpu().numpy(), status.cpu().numpy(), want, f"golden {feature}")


def test_normalize_is_numpy_float64_rounded_once(synth, golden_corpus, device):
    """``normalize_()``: the corpus arrays equal ``((x64 - mean) / std).astype(float32)`` bit for bit with the device's
    own mean and std; ``batch`` of a variant plan carries those values at sigma; a second call raises."""
    g, make = golden_corpus
    corpus = make()
    names, plan = corpus.variants(g["cfg_b"])
    raw = {f: corpus.tensors["ch_" + f].cpu().numpy().copy() for f in S.FEATURES}
    assert not corpus.normalized
    st = corpus.normalize_(cfg=g["cfg_b"])
    assert corpus.normalized and st == make().stats(plan) and corpus.last_status.tolist() == [0] * 60
    normed = {}
    for f in S.FEATURES:
        mean, std = np.float64(st[f][2]), np.float64(st[f][3])
        normed[f] = ((raw[f].astype(np.float64) - mean) / std).astype(np.float32)
        got = corpus.tensors["ch_" + f].cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), normed[f].view(np.int32)), f
        assert not np.array_equal(got, raw[f])
    pick = [i for i, n in enumerate(names) if n.endswith(("-consecutive2", "-repeat3", "-firstconsecutive1"))][:8]
    batch = corpus.batch(plan[pick])
    off = np.concatenate([[0], np.cumsum(corpus.n_chars)])
    for b, (src, pos, m, _, r) in enumerate(plan[pick].tolist()):
        sg = off[src] + C.sigma(corpus.n_chars[src], pos, m, r)
        for f, i in (("energy", 8), ("kurtosis", 9)):
            row = batch[i][b].cpu().numpy()
            assert np.array_equal(row[:len(sg)].view(np.int32), normed[f][sg].view(np.int32)) and not row[len(sg):].any()
    with pytest.raises(ValueError, match="already normalised"):
        corpus.normalize_(cfg=g["cfg_b"])
    with pytest.raises(ValueError, match="already normalised"):
        corpus.normalize_(stats=st)
    other = make()  # given statistics: the same values
    assert other.normalize_(stats=st) == st
    for f in S.FEATURES:
        assert torch.equal(other.tensors["ch_" + f], corpus.tensors["ch_" + f])
    with pytest.raises(ValueError, match="not both"):
        make().normalize_(stats=st, cfg=g["cfg_b"])


def test_graph_replay_follows_a_plan_rewritten_in_place(synth, device):
    """Statistics and normalisation of a copy of the energies captured in one graph with a device plan: a replay
    after the plan was rewritten in place gives the new plan's statistics and the values normalised by them."""
    import visual_onoma_to_wave_amd  # noqa: F401  (before the first GPU call: its import-time runtime setting)
    from visual_onoma_to_wave_amd import ops
    corpus, values = synth
    first, second = EDGES[6:16], [EDGES[11], EDGES[3], EDGES[39], EDGES[20], EDGES[30]] * 2
    assert len(first) == len(second)
    plan_d = torch.tensor(first, dtype=torch.int32, device=device)
    raw = corpus.tensors["ch_energy"].clone()
    work = raw.clone()
    out, status = ops.corpus_stats(corpus.struct, plan_d, "energy")  # warm outside the capture; the static tensors
    ws = torch.empty(len(first) * 40, dtype=torch.uint8, device=device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.corpus_stats(corpus.struct, plan_d, "energy", out=out, status=status, workspace=ws)
        ops.corpus_normalize_(work, out)
    for plan in (second, first):
        plan_d.copy_(torch.tensor(plan, dtype=torch.int32, device=device))
        work.copy_(raw)  # the values are restored between replays
        graph.replay()
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        _check(o, status.cpu().numpy(), S.model(values["energy"], plan), f"graph replay, {len(plan)} rows")
        want = ((raw.cpu().numpy().astype(np.float64) - o[1]) / o[2]).astype(np.float32)
        assert np.array_equal(work.cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(corpus.tensors["ch_energy"], raw)  # the corpus itself was never written


def test_end_to_end_on_the_golden(golden_corpus, device):
    """A raw corpus + ``variants(cfg)`` + ``normalize_()`` against ``normalize_features(remove_outlier=True)`` over the
    golden's materialised arrays (its 53 variant files and their 7 bases, as float32: what the corpus packs and what
    ``to_device`` makes of a file): the statistics within the bar, and every file's normalised energy and kurtosis,
    rounded to float32, equal to the device's values at the file's characters."""
    from visual_onoma_to_wave_amd.preprocessor import normalize_features
    g, make = golden_corpus
    corpus = make()
    names, plan = corpus.variants(g["cfg_b"])
    files = {u["id"]: u for u in g["bases"] + g["variants"]}
    assert len(names) == 60 and len(g["variants"]) == 53
    st = corpus.normalize_(cfg=g["cfg_b"])
    off = np.concatenate([[0], np.cumsum(corpus.n_chars)])
    for f in S.FEATURES:
        arrays = [files[n][f].astype(np.float32).astype(np.float64) for n in names]
        normed, mean, std, mn, mx = normalize_features(arrays, remove_outlier=True)
        n_kept = sum(len(k) for k in S.load()[f"{f}_f32_kept"])
        bm, bs = S.bar({"count": n_kept, "mean": mean, "std": std})
        assert abs(st[f][2] - mean) <= bm and abs(st[f][3] - std) <= bs
        for got, want in ((st[f][0], mn), (st[f][1], mx)):  # (x - mean) / std with mean and std moved by their bars
            assert abs(got - want) <= (bm + abs(want) * bs) / std + 4 * np.spacing(abs(want)), (f, got, want)
        dev = corpus.tensors["ch_" + f].cpu().numpy()
        for name, (src, pos, m, _, r), v in zip(names, plan.tolist(), normed):
            sg = off[src] + C.sigma(corpus.n_chars[src], pos, m, r)
            assert np.array_equal(dev[sg].view(np.int32), v.astype(np.float32).view(np.int32)), (f, name)
