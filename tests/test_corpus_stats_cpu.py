"""The corpus statistics on the host: the numpy model of tests/corpus_stats_check.py and
``preprocessor.normalize_features(remove_outlier=True)`` against the reference's own ``_remove_outlier`` and
``StandardScaler`` (tests/golden/corpus_stats.npz), the unchanged default of ``normalize_features``, and the plan
rules.  The GPU tests hold the kernels against the same model."""

import numpy as np
import pytest

import augment_check as C
import corpus_stats_check as S


@pytest.fixture(scope="module")
def g():
    return C.load()


@pytest.fixture(scope="module")
def gs():
    return S.load()


def base_values(g, feature):
    return [u[feature].astype(np.float32) for u in g["bases"]]


def within_bar(got_mean, got_std, want):
    bm, bs = S.bar(want)
    return abs(got_mean - want["mean"]) / bm, abs(got_std - want["std"]) / bs


@pytest.mark.parametrize("feature", S.FEATURES)
def test_model_keeps_what_the_reference_keeps(g, gs, feature):
    """Every golden file as a plan row over the base utterances: the row's array under sigma, filtered, is the
    reference's ``_remove_outlier`` of the file element for element; mean and std over all files are
    ``StandardScaler``'s within the summation bound."""
    names, plan = S.golden_plan(g)
    assert len(names) == 60 and sorted(names) == sorted(v["id"] for v in g["bases"] + g["variants"])
    m = S.model(base_values(g, feature), plan)
    assert m["status"].tolist() == [0] * 60
    for name, got, want in zip(names, m["kept"], gs[f"{feature}_f32_kept"]):
        assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), name
    assert sum(len(k) == 0 for k in m["kept"]) >= 1  # the one-character utterance keeps nothing and is skipped
    mean, scale = gs[f"{feature}_f32_scaler"]
    rm, rs = within_bar(mean, scale, m)
    print(f"{feature}: model against StandardScaler, ratio to the bar: mean {rm:.3f}, std {rs:.3f}")
    assert rm <= 1 and rs <= 1 and m["margin"] > 1e-9


@pytest.mark.parametrize("feature", S.FEATURES)
def test_float64_files_and_hand_made_arrays(g, gs, feature):
    """The files as the reference wrote them (float64) and the hand-made edge cases, through ``keep`` and through
    the package's ``iqr_inliers``."""
    from visual_onoma_to_wave_amd.preprocessor.features import iqr_inliers
    files = {u["id"]: u[feature] for u in g["bases"] + g["variants"]}
    for name, want in zip(gs["names"], gs[f"{feature}_f64_kept"]):
        assert np.array_equal(S.keep(files[name]), want) and np.array_equal(iqr_inliers(files[name]), want), name
    kept = dict(zip(gs["hand_names"], gs["hand_kept"]))
    for name, v, want in zip(gs["hand_names"], gs["hand"], gs["hand_kept"]):
        assert np.array_equal(S.keep(v), want) and np.array_equal(iqr_inliers(v), want), name
    for name in ("one", "equal"):
        assert len(kept[name]) == 0, name
    assert kept["quartiles_coincide"].size == 0 and 13.0 not in kept["on_the_upper_fence"]
    assert len(kept["on_the_upper_fence"]) == 8 and len(kept["far_outliers"]) == 30


@pytest.mark.parametrize("feature", S.FEATURES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_normalize_features_with_the_outlier_rule(g, gs, feature, prec):
    from visual_onoma_to_wave_amd.preprocessor import normalize_features
    files = {u["id"]: u[feature] for u in g["bases"] + g["variants"]}
    arrays = [files[n] if prec == "f64" else files[n].astype(np.float32).astype(np.float64) for n in gs["names"]]
    normed, mean, std, mn, mx = normalize_features(arrays, remove_outlier=True)
    want_mean, want_std = gs[f"{feature}_{prec}_scaler"]
    n = sum(len(k) for k in gs[f"{feature}_{prec}_kept"])
    ref = {"count": n, "mean": want_mean, "std": want_std}
    rm, rs = within_bar(mean, std, ref)
    print(f"{feature} {prec}: normalize_features against StandardScaler, ratio to the bar: mean {rm:.3f}, std {rs:.3f}")
    assert rm <= 1 and rs <= 1
    for a, v in zip(arrays, normed):  # every value is normalised, outliers included
        assert np.array_equal(v, (a - mean) / std)
    assert mn == min(float(v.min()) for v in normed) and mx == max(float(v.max()) for v in normed)
    _, mean0, std0, _, _ = normalize_features(arrays)
    assert (mean0, std0) != (mean, std)  # the rule matters on this corpus


def test_normalize_features_default_is_unchanged():
    """``remove_outlier=False`` against a literal recomputation of what the function did before the argument."""
    from visual_onoma_to_wave_amd.preprocessor import normalize_features
    rng = np.random.default_rng(7)
    for arrays in ([rng.standard_normal(n) * 3 + 1 for n in (1, 5, 17, 2)] + [np.array([40.0])],
                   [rng.standard_normal(n).astype(np.float32) for n in (3, 8)],
                   [np.full(4, 2.5)]):
        flat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in arrays])
        mean = float(flat.mean())
        std = float(np.sqrt(np.mean((flat - mean) ** 2)))
        std = 1.0 if std == 0.0 else std
        want = [(np.asarray(a) - mean) / std for a in arrays]
        for got in (normalize_features(arrays), normalize_features(arrays, remove_outlier=False)):
            assert got[1] == mean and got[2] == std
            assert got[3] == min(float(np.min(v)) for v in want) and got[4] == max(float(np.max(v)) for v in want)
            for a, b in zip(got[0], want):
                assert a.dtype == b.dtype and np.array_equal(a, b)
    with pytest.raises(ValueError, match="keeps no value"):
        normalize_features([np.full(4, 2.5), np.array([1.0])], remove_outlier=True)


def test_plan_rules(g):
    """The range rules of a host plan (``check_plan`` without caps: what ``DeviceCorpus.stats`` applies) and the
    model's status codes, which are the device's."""
    from visual_onoma_to_wave_amd import _lib
    from visual_onoma_to_wave_amd.preprocessor import augment as AU
    assert (S.OK, S.BAD_ROW, S.CHARS_OVER, S.MAX_CHARS) == (_lib.AUG_OK, _lib.AUG_BAD_ROW, _lib.STATS_CHARS_OVER,
                                                            _lib.STATS_MAX_CHARS)
    assert _lib.STATS_CHARS_OVER not in (_lib.AUG_CHARS_OVER, _lib.AUG_FRAMES_OVER)
    n_chars = [len(u["text"]) for u in g["bases"]]
    n_frames = [int(u["duration"].sum()) for u in g["bases"]]
    durs = [u["duration"] for u in g["bases"]]
    for row, rule in (((7, 0, 0, 0, 1), "src is outside"), ((-1, 0, 0, 0, 1), "src is outside"),
                      ((2, 4, 0, 0, 1), "pos is outside"), ((2, -1, 0, 0, 1), "pos is outside"),
                      ((0, 0, -1, 0, 1), "m and m_mel"), ((0, 0, 0, -1, 1), "m and m_mel"),
                      ((0, 0, 0, 0, 0), "m and m_mel")):
        with pytest.raises(ValueError, match=f"plan row 1 .*{rule}"):
            AU.check_plan([(0, 0, 0, 0, 1), row], n_chars, n_frames, durs)
        assert S.row_status(n_chars, row) == S.BAD_ROW
    # no cap on the host: a row over VO_STATS_MAX_CHARS passes the range rules and is refused on the device
    over = (0, 0, 0, 0, S.MAX_CHARS // 2 + 1)
    p, src_lens, _ = AU.check_plan([over, (0, 0, 0, 0, S.MAX_CHARS // 2)], n_chars, n_frames, durs)
    assert src_lens == [S.MAX_CHARS + 2, S.MAX_CHARS] and p.dtype == np.int32
    assert [S.row_status(n_chars, r) for r in p.tolist()] == [S.CHARS_OVER, S.OK]
    assert S.row_status(n_chars, (0, 0, 2 ** 31 - 1, 0, 2 ** 31 - 1)) == S.CHARS_OVER
    # a one-character utterance keeps nothing but still counts for min / max; refused rows count for neither
    m = S.model([u["energy"].astype(np.float32) for u in g["bases"]], [(1, 0, 0, 0, 1), (9, 0, 0, 0, 1), over])
    assert m["status"].tolist() == [0, 1, 4] and m["count"] == 0 and (m["mean"], m["std"]) == (0.0, 1.0)
    assert m["raw_min"] == m["raw_max"] == float(g["bases"][1]["energy"].astype(np.float32)[0]) and m["rows_used"] == 0


def test_ops_refuse_host_tensors():
    """The argument checks of the two ops come before the library is touched."""
    import torch
    from visual_onoma_to_wave_amd import _lib, ops
    corpus = _lib.Corpus(U=1)
    with pytest.raises(ValueError, match="plan must be an int32"):
        ops.corpus_stats(corpus, torch.zeros((2, 5), dtype=torch.int32), "energy")
    with pytest.raises(ValueError, match="values must be a non-empty fp32 tensor on the GPU"):
        ops.corpus_normalize_(torch.zeros(3), torch.zeros(6, dtype=torch.float64))
