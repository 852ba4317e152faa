"""CPU tests of the score statistics: the curve arithmetic of kws_amd.metrics on hand-made count arrays (no device), the numpy reference
against its own plain-loop form, the host-only path predicate of kws_score_hist, and eval.py's new flags."""
import os
import re
import warnings

import numpy as np
import pytest

import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats_of(hist, rank_counts=None, calib=None):
    from kws_amd.metrics import ScoreStats
    hist = np.asarray(hist, np.int64)
    C, _, bins = hist.shape
    rank_counts = np.zeros((C,), np.int64) if rank_counts is None else rank_counts
    calib = np.zeros((2, bins), np.int64) if calib is None else calib
    return ScoreStats.from_counts(hist, rank_counts, calib)


# ---- the reference itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [2, 8, 1024, 65536])
def test_binning_rule_edges(bins):
    one = np.float32(1)
    p = np.array([0.0, -0.0, -3.5, np.nan, 1.0, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), 7.0, np.inf, -np.inf,
                  np.float32(1e-45), 0.5, np.nextafter(np.float32(0.5), np.float32(0))], np.float32)
    want = [0, 0, 0, 0, bins - 1, bins - 1, bins - 1, bins - 1, bins - 1, 0, 0, bins // 2, bins // 2 - 1]
    assert score_ref.score_bin(p, bins).tolist() == want
    j = np.arange(bins, dtype=np.float32) / np.float32(bins)                     # exact in fp32 for power-of-two bins
    assert score_ref.score_bin(j, bins).tolist() == list(range(bins))
    below = np.nextafter(j[1:], np.float32(0))
    assert score_ref.score_bin(below, bins).tolist() == list(range(bins - 1))


def test_vectorised_reference_equals_plain_loops():
    rng = np.random.default_rng(3)
    for C, bins in [(2, 2), (3, 8), (12, 16)]:
        p = rng.dirichlet(np.ones(C) * 0.3, 90).astype(np.float32)
        p[5] = p[5, 0]                                                           # all equal: rank by index
        p[6, C - 1] = np.nan
        p[7] = 0.0
        p[8, 0] = 1.0
        y = rng.integers(-1, C + 2, 90)
        got, want = score_ref.score_counts(p, y, bins), score_ref.score_counts_loops(p, y, bins)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        valid = int(((y >= 0) & (y < C)).sum())
        assert got[1].sum() == valid and got[2][0].sum() == valid and got[0].sum() == valid * C
        assert got[2][1].sum() == got[1][0]


# ---- curve arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_auc_is_the_pairwise_value(seed):
    rng = np.random.default_rng(seed)
    C, bins = 5, 24
    hist = rng.integers(0, 50, (C, 2, bins))
    hist[1, :, rng.integers(0, bins, 10)] = 0                                    # empty bins
    hist[2, 1, :12] = 0                                                          # targets high only
    auc = stats_of(hist).auc()
    for c in range(C):
        assert abs(auc[c] - score_ref.pairwise_auc(hist[c, 1], hist[c, 0])) <= 1e-12


def test_auc_survives_counts_past_2_to_31():
    hist = np.zeros((1, 2, 4), np.int64)
    hist[0, 1] = [0, 1 << 33, 0, 3 << 33]
    hist[0, 0] = [5 << 33, 1 << 33, 1 << 33, 0]
    got = stats_of(hist).auc()[0]
    assert abs(got - score_ref.pairwise_auc(hist[0, 1], hist[0, 0])) <= 1e-12
    cv = stats_of(hist).curves()
    assert cv["tpr"][0].tolist() == [1.0, 1.0, 0.75, 0.75, 0.0]


def test_perfectly_separated_scores():
    bins = 16
    hist = np.zeros((2, 2, bins), np.int64)
    hist[0, 0, :5] = [7, 3, 1, 0, 2]
    hist[0, 1, 9:] = 4
    hist[1, 0, 0] = 11                                                           # adjacent bins still separate
    hist[1, 1, 1] = 5
    s = stats_of(hist)
    np.testing.assert_array_equal(s.auc(), [1.0, 1.0])
    eer, thr = s.eer()
    np.testing.assert_array_equal(eer, [0.0, 0.0])
    assert 5 / bins <= thr[0] <= 9 / bins and thr[1] == 1 / bins
    where, miss = s.at_far(0.0)
    assert where.tolist() == [5 / bins, 1 / bins] and miss.tolist() == [0.0, 0.0]


def test_identical_distributions():
    bins = 8
    hist = np.zeros((3, 2, bins), np.int64)
    hist[0, :, :] = 6                                                            # uniform
    hist[1, 0] = hist[1, 1] = [9, 0, 4, 4, 1, 0, 0, 30]
    hist[2, :, 3] = 17                                                           # everything in one bin
    s = stats_of(hist)
    np.testing.assert_allclose(s.auc(), 0.5, rtol=0, atol=1e-12)
    eer, thr = s.eer()
    np.testing.assert_allclose(eer, 0.5, rtol=0, atol=1e-12)
    assert abs(thr[0] - 0.5) < 1e-12 and abs(thr[2] - 3.5 / bins) < 1e-12


def test_curves_and_at_far_take_the_lowest_admissible_threshold():
    bins = 4
    hist = np.zeros((1, 2, bins), np.int64)
    hist[0, 0] = [90, 6, 3, 1]                                                   # fpr at j = 0..4: 1, .1, .04, .01, 0
    hist[0, 1] = [1, 1, 2, 6]                                                    # frr at j = 0..4: 0, .1, .2, .4, 1
    s = stats_of(hist)
    cv = s.curves()
    np.testing.assert_allclose(cv["thresholds"], [0, .25, .5, .75, 1])
    np.testing.assert_allclose(cv["fpr"][0], [1, .1, .04, .01, 0], atol=1e-15)
    np.testing.assert_allclose(cv["tpr"][0], [1, .9, .8, .6, 0], atol=1e-15)
    np.testing.assert_allclose(cv["frr"][0], [0, .1, .2, .4, 1], atol=1e-15)
    for far, j in [(1.0, 0), (0.5, 1), (0.1, 1), (0.0999, 2), (0.04, 2), (0.02, 3), (0.01, 3), (0.005, 4), (0.0, 4)]:
        where, miss = s.at_far(far)
        assert where[0] == j / bins and abs(miss[0] - cv["frr"][0, j]) < 1e-15, far
    eer, thr = s.eer()                                                           # frr - fpr: -1, 0, ...: the crossing is at j = 1
    assert abs(eer[0] - 0.1) < 1e-12 and abs(thr[0] - 0.25) < 1e-12


def test_eer_interpolates_between_thresholds():
    hist = np.zeros((1, 2, 2), np.int64)                                         # the single-threshold edge: bins = 2
    hist[0, 0] = [3, 1]                                                          # fpr: 1, .25, 0
    hist[0, 1] = [1, 4]                                                          # frr: 0, .2, 1
    eer, thr = stats_of(hist).eer()
    # d = frr - fpr: -1, -0.05, 1: crossing between j = 1 and 2 at a = 0.05 / 1.05
    a = 0.05 / 1.05
    assert abs(eer[0] - (0.2 + a * 0.8)) < 1e-12 and abs(thr[0] - (0.5 + a * 0.5)) < 1e-12
    where, miss = stats_of(hist).at_far(0.0)
    assert where[0] == 1.0 and miss[0] == 1.0                                    # only "detect nothing" has no false accepts
    where, miss = stats_of(hist).at_far(0.25)
    assert where[0] == 0.5 and abs(miss[0] - 0.2) < 1e-15


def test_class_without_targets_or_non_targets_is_nan_silently():
    hist = np.zeros((3, 2, 8), np.int64)
    hist[0, 0, 2] = 5                                                            # no targets
    hist[1, 1, 6] = 5                                                            # no non-targets
    hist[2, 0, 1] = hist[2, 1, 5] = 3
    s = stats_of(hist)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        auc, (eer, thr), (where, miss), cv = s.auc(), s.eer(), s.at_far(0.01), s.curves()
        empty = stats_of(np.zeros((2, 2, 4), np.int64))
        assert np.isnan(empty.top_k(1)) and np.isnan(empty.ece()[0]) and np.isnan(empty.auc()).all()
    for v in (auc, eer, thr, where, miss):
        assert np.isnan(v[0]) and np.isnan(v[1]) and v[2] == v[2]
    assert np.isnan(cv["tpr"][0]).all() and not np.isnan(cv["fpr"][0]).any()
    assert np.isnan(cv["fpr"][1]).all() and not np.isnan(cv["tpr"][1]).any()


def test_top_k_is_the_cumulative_rank_count():
    rank = np.array([60, 25, 10, 0, 5], np.int64)
    s = stats_of(np.zeros((5, 2, 4), np.int64), rank_counts=rank)
    assert [s.top_k(k) for k in (1, 2, 3, 4, 5)] == [0.6, 0.85, 0.95, 0.95, 1.0]
    assert s.top_k(9) == 1.0 and s.top_k(0) == 0.0
    big = stats_of(np.zeros((2, 2, 4), np.int64), rank_counts=np.array([3 << 40, 1 << 40], np.int64))
    assert big.top_k(1) == 0.75 and big.top_k(2) == 1.0


def test_ece_and_reliability_table():
    bins = 4
    calib = np.array([[0, 10, 0, 30], [0, 5, 0, 27]], np.int64)
    ece, table = stats_of(np.zeros((2, 2, bins), np.int64), calib=calib).ece()
    want = (10 * abs(0.5 - 0.375) + 30 * abs(0.9 - 0.875)) / 40
    assert abs(ece - want) < 1e-12
    np.testing.assert_array_equal(table["count"], calib[0])
    np.testing.assert_allclose(table["confidence"], [.125, .375, .625, .875])
    assert np.isnan(table["accuracy"][[0, 2]]).all() and table["accuracy"][1] == 0.5 and table["accuracy"][3] == 0.9
    # a perfectly calibrated bin still shows the half-bin resolution, and no more
    calib = np.array([[0, 0, 0, 8], [0, 0, 0, 7]], np.int64)
    assert stats_of(np.zeros((2, 2, bins), np.int64), calib=calib).ece()[0] == 0.0


def test_merge_adds_and_checks_the_shape():
    rng = np.random.default_rng(1)
    a = [rng.integers(0, 9, s) for s in [(3, 2, 8), (3,), (2, 8)]]
    b = [rng.integers(0, 9, s) for s in [(3, 2, 8), (3,), (2, 8)]]
    from kws_amd.metrics import ScoreStats
    sa, sb = ScoreStats.from_counts(*a), ScoreStats.from_counts(*b)
    assert sa.merge(sb) is sa
    for got, x, y in zip(sa.counts(), a, b):
        np.testing.assert_array_equal(got, x + y)
        assert got.dtype == np.int64
    for got, y in zip(sb.counts(), b):
        np.testing.assert_array_equal(got, y)
    with pytest.raises(ValueError):
        sa.merge(stats_of(np.zeros((3, 2, 4), np.int64)))
    with pytest.raises(ValueError):
        ScoreStats.from_counts(a[0], a[1][:2], a[2])


# ---- the library's host-only predicate ----------------------------------------------------------------------------------------
def header_budget():
    text = open(os.path.join(ROOT, "include", "kws.h")).read()
    return int(re.search(r"#define\s+KWS_SCORE_LDS_BUDGET\s+(\d+)", text).group(1))


def test_uses_lds_agrees_with_the_header_and_is_monotone():
    from kws_amd.metrics import uses_lds
    budget = header_budget()
    assert 8 * 12 * 1024 <= budget <= 160 * 1024                                # the default evaluation fits; a block fits a compute unit
    shapes = [(C, bins) for C in (1, 2, 3, 12, 35, 64, 65, 1024) for bins in (2, 3, 12, 512, 1023, 1024, 1025, 4096, 6144, 6145, 65536)]
    for C, bins in shapes:
        assert uses_lds(C, bins) == (8 * C * bins <= budget), (C, bins)
    order = sorted(shapes, key=lambda s: s[0] * s[1])
    flags = [uses_lds(*s) for s in order]
    assert flags == sorted(flags, reverse=True) and flags[0] and not flags[-1]
    edge = budget // 16                                                          # bins at C = 2 on either side of the budget
    assert uses_lds(2, edge) and not uses_lds(2, edge + 1)
    assert uses_lds(12, 1024) and not uses_lds(13, 1024)
    assert not uses_lds(0, 1024) and not uses_lds(12, 1)


def test_score_hist_rejects_bad_arguments_on_the_host():
    from kws_amd import lib as l
    L = l.get_lib()
    buf = (np.zeros(64, np.int64)).ctypes.data
    for args in [(0, buf, 1, 2, 4, buf), (buf, 0, 1, 2, 4, buf), (buf, buf, 1, 2, 4, 0), (buf, buf, -1, 2, 4, buf), (buf, buf, 1, 0, 4, buf),
                 (buf, buf, 1, 2, 1, buf)]:
        assert L.kws_score_hist(*args, None, None, None) == l.ERR_INVALID, args
    assert L.kws_score_hist(buf, buf, 0, 2, 4, buf, None, None, None) == 0      # B == 0: nothing is launched


# ---- eval.py ------------------------------------------------------------------------------------------------------------------
def test_eval_parse_args_takes_the_new_flags():
    import eval as kws_eval
    base = ["--weights_path", "w.npz", "--dataset_path", "d", "--classes_path", "c.txt"]
    a = kws_eval.parse_args(base)
    assert a.curves is False and a.bins == 1024 and a.max_far == 0.01 and a.top_k == 3 and a.curves_csv is None
    a = kws_eval.parse_args(base + ["--curves", "--bins", "256", "--max_far", "0.05", "--top_k", "5", "--curves_csv", "roc.csv", "--int8"])
    assert a.curves is True and a.bins == 256 and a.max_far == 0.05 and a.top_k == 5 and a.curves_csv == "roc.csv" and a.int8
    for bad in (["--curves", "--bins", "1"], ["--curves", "--top_k", "0"], ["--curves", "--max_far", "1.5"], ["--curves_csv", "roc.csv"]):
        with pytest.raises(SystemExit):
            kws_eval.parse_args(base + bad)


def test_score_table_and_csv_print_from_host_counts(tmp_path, capsys):
    import eval as kws_eval
    rng = np.random.default_rng(0)
    C, bins, names = 3, 8, ["background", "yes", "no"]
    p = rng.dirichlet(np.ones(C), 200).astype(np.float32)
    y = rng.integers(0, C, 200)
    from kws_amd.metrics import ScoreStats
    s = ScoreStats.from_counts(*score_ref.score_counts(p, y, bins))
    kws_eval.print_score_table(s, names, 0.05, 2)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 + C + 2 and out[0].split()[:3] == ["class", "targets", "non-targets"]
    assert out[1].split()[0] == "background" and int(out[1].split()[1]) == int((y == 0).sum()) and int(out[1].split()[2]) == int((y != 0).sum())
    assert out[-2].startswith("top-1 accuracy") and "top-2 accuracy" in out[-2] and "top-3" not in out[-2] and out[-1].startswith("ECE ")
    kws_eval.print_score_table(s, names, 0.05, 1, title="int8:", baseline=s)       # beside a baseline: the differences, here all zero
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "int8:" and out[1].split()[-2:] == ["EER-fp32", "miss-fp32"] and len(out) == 2 + C + 2
    assert all(row.split()[-2:] == ["+0.0000", "+0.0000"] for row in out[2:2 + C])
    path = str(tmp_path / "roc.csv")
    kws_eval.write_curves_csv(path, s, names)
    rows = open(path).read().splitlines()
    assert rows[0] == "class,threshold,tpr,fpr" and len(rows) == 1 + C * (bins + 1)
    first, last = rows[1].split(","), rows[bins + 1].split(",")
    assert first == ["background", "0", "1", "1"] and last == ["background", "1", "0", "0"]
