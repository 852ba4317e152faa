"""Host-side checks of the optimizer edge table (tests/optim_edge_cases.py): the block table kws_optimizer_plan makes of it, the
branches the table and the case list exist for, the float32 restatement of csrc/kws_optim.hip against the float64 oracle on every case,
and the oracle's non-finite rules worked by hand on the 3-float and 5-float segments.  No GPU."""
import numpy as np
import pytest

import optim_edge_cases as ec
from optim_ref import RefOptimizer


def test_the_table_is_laid_out_as_documented():
    assert ec.SIZES == [1, 2, 3, 5, 1023, 1024, 1025, 2051, 262145, 263171]
    assert ec.OFFSETS[0] == 4 and all(o % 4 == 0 for o in ec.OFFSETS)
    ends = [o + n for o, n in ec.SEGMENTS]
    assert all(8 <= o - e <= 11 for o, e in zip(ec.OFFSETS[1:], ends))          # 8 floats, plus what rounds the end up to a multiple of 4
    assert 4 <= ec.TOTAL - ends[-1] <= 7 and ec.TOTAL % 4 == 0
    assert ec.INSIDE.sum() == sum(ec.SIZES) == 530450 and not ec.INSIDE[:4].any() and not ec.INSIDE[-4:].any()
    assert 4 * ec.TOTAL < 2.2e6                                                # 2 MB per buffer


def test_planned_block_table_of_the_edge_table():
    host, nb, tab = ec.plan(ec.OFFSETS, ec.SIZES)
    assert ec.BLOCKS == [1, 1, 1, 1, 1, 1, 2, 3, 257, 258] and nb == ec.N_BLOCKS == 526
    assert host.nbytes == (32 * nb + 255) // 256 * 256 + 8 * nb
    assert not host[32 * nb:].any()
    assert (tab["begin"] % 4 == 0).all() and (tab["reserved"] == 0).all()
    k = 0
    for s, ((o, n), count) in enumerate(zip(ec.SEGMENTS, ec.BLOCKS)):
        rows = tab[k:k + count]
        assert (rows["seg"] == s).all() and (rows["first"] == k).all() and (rows["count"] == count).all()
        assert rows["begin"].tolist() == [o + 1024 * j for j in range(count)]
        assert rows["end"][:-1].tolist() == [o + 1024 * (j + 1) for j in range(count - 1)] and rows["end"][-1] == o + n
        assert (rows["begin"] >= o).all() and (rows["end"] <= o + n).all() and (rows["begin"] < rows["end"]).all()
        k += count
    assert k == nb
    last = [int(tab["end"][k] - tab["begin"][k]) for k in np.cumsum(ec.BLOCKS) - 1]
    assert last == [1, 2, 3, 5, 1023, 1024, 1, 3, 1, 3]
    # the blocks tile the inside of the segments and nothing else
    hit = np.zeros((ec.TOTAL,), np.int32)
    for b, e in zip(tab["begin"], tab["end"]):
        hit[b:e] += 1
    np.testing.assert_array_equal(hit, ec.INSIDE.astype(np.int32))


def test_required_branches_are_covered():
    got = ec.covered()
    assert ec.REQUIRED <= got, ec.REQUIRED - got
    assert len([r for r in ec.REQUIRED if isinstance(r, tuple) and r[0] == "combo"]) == 27
    # sizes: every size % 4, a block of one float behind 256 full ones, a full block and a tail of 3 behind them
    assert {n % 4 for n in ec.SIZES} == {0, 1, 2, 3}
    assert 262145 == 256 * 1024 + 1 and 263171 == 257 * 1024 + 3
    assert sorted(b for b in ec.BLOCKS if b > ec.SUM_STRIDE) == [257, 258] and ec.N_BLOCKS > 2 * ec.SUM_STRIDE


def test_the_case_list_turns_every_option_on():
    labels = [c.label for c in ec.CASES]
    assert len(set(labels)) == len(labels)
    full = [c for c in ec.CASES if dict(c.options) == ec.FLAGS_ON[c.kind]]
    assert {(c.kind, c.norm, c.avg) for c in full} == {(k, n, a) for k in ec.KINDS for n in ec.NORMS for a in ec.AVGS}
    for c in full:
        assert ec.slots_of(c) == {"sgd": ("mom",), "rmsprop": ("v", "mg", "mom"), "adam": ("m", "v", "vhat")}[c.kind]
    assert all(c.steps >= 3 for c in ec.CASES)
    assert {c.grad_scale for c in ec.CASES} == {1.0, 0.5, 1.0 / 128}
    assert any(c.grad_scale != 1.0 and c.norm == n for c in ec.CASES for n in ("var", "global"))
    clipped = sum(1 for c in ec.CASES if c.clipvalue > 0)
    assert 0.4 <= clipped / len(ec.CASES) <= 0.6
    assert any(c.kind == "adam" and c.t0 == 1 for c in ec.CASES) and any(c.kind == "adam" and c.t0 == 10 ** 6 for c in ec.CASES)
    assert {c.norm for c in ec.CASES if c.pattern == "huge"} == {"var", "global"}
    assert all(c.clipvalue == 0 for c in ec.CASES if c.pattern == "huge")
    assert all(c.pattern in ("tail_heavy", "huge") for c in full if c.norm != "none")          # huge is tail_heavy but for one segment
    assert ec.slots_of(ec.CASE["sgd-plain"]) == () and ec.slots_of(ec.CASE["rmsprop-plain"]) == ("v",)


def test_tail_heavy_gradients_put_the_norm_on_the_edges():
    moves = []
    for step in range(3):
        g = ec.gradient("tail_heavy", step).astype(np.float64)
        assert np.isnan(g[~ec.INSIDE]).all() and np.isfinite(g[ec.INSIDE]).all()
        total = float(np.sum(g[ec.INSIDE] ** 2))
        far, beyond = 0.0, 0.0
        k = 0
        for s, ((o, n), count) in enumerate(zip(ec.SEGMENTS, ec.BLOCKS)):
            x = g[o:o + n]
            sq = float(np.sum(x * x))
            if s == ec.zero_segment(step):
                assert not x.any()
            else:
                np.testing.assert_allclose(np.sqrt(sq), 3.0 if (s + step) % 2 == 0 else 0.3, rtol=1e-6)
                tail = n % 4 or 1
                assert np.sum(x[n - tail:] ** 2) > (0.29 if n == 263171 else 0.5) * sq     # 263171: half of the 60 % lies on block 256
                if count > 256:
                    assert np.sum(x[256 * 1024:] ** 2) > 0.5 * sq
                    assert np.sum(x[:256 * 1024] ** 2) > 0.3 * sq
            for j in range(count):                     # the squared norm behind global blocks 256 and 512
                part = float(np.sum(x[1024 * j:1024 * (j + 1)] ** 2))
                far += part if k + j >= 256 else 0.0
                beyond += part if k + j >= 512 else 0.0
            k += count
        print("step %d: blocks >= 256 hold %.3g of the squared norm, blocks >= 512 %.3g" % (step, far / total, beyond / total))
        moves.append((1.0 - np.sqrt(1.0 - far / total), 1.0 - np.sqrt(1.0 - beyond / total)))
    # a global sum that drops either moves the scale by more than 50 times the tolerance at every step (the last segment has norm 0.3 at
    # the even steps, against 6.7 over the table) and by more than 1000 times at the odd ones
    assert min(min(m) for m in moves) > 50 * ec.PARAM_RTOL and min(moves[1]) > 1000 * ec.PARAM_RTOL
    g = ec.gradient("huge", 0)
    o, n = ec.SEGMENTS[ec.HUGE_SEGMENT]
    with np.errstate(over="ignore"):
        assert (np.abs(g[o:o + n]) == np.float32(ec.HUGE)).all() and np.isinf(np.float32(ec.HUGE) * np.float32(ec.HUGE))
    # every segment is all zeros at one of the steps 0 .. 2 at most once, and the zero segments differ in size % 4 and block count
    assert [ec.SIZES[ec.zero_segment(s)] for s in range(3)] == [2, 1025, 262145]


def test_raw_gradients_undo_grad_scale_exactly():
    scaled = [c for c in ec.CASES if c.grad_scale != 1.0]
    assert {c.pattern for c in scaled} == {"decades", "tail_heavy", "huge"}
    for c in scaled[:2] + [ec.CASE["adam-global-huge"]]:
        for raw, g in zip(ec.raw_gradients(c), ec.gradients(c)):
            np.testing.assert_array_equal(raw[ec.INSIDE] * np.float32(c.grad_scale), g[ec.INSIDE])


_WORST = {}


def _worst_ratios(case):
    """the float32 restatement against the float64 oracle after every step of the case, as the largest error / bound per buffer class;
    computed once per case"""
    if case.label in _WORST:
        return _WORST[case.label]
    worst = {"params": 0.0, "slots": 0.0, "avg": 0.0}
    outside = ec.start("p")[~ec.INSIDE]
    steps = 0
    for (p, avg, slots), (pr, avgr, slotsr) in zip(ec.run_float32(case), ec.run_oracle(case)):
        assert np.array_equal(p[~ec.INSIDE], outside) and np.array_equal(pr[~ec.INSIDE], outside)
        worst["params"] = max(worst["params"], ec.bound_ratio(p, pr, ec.PARAM_RTOL, ec.PARAM_ATOL))
        assert set(slots) == set(slotsr) == set(ec.slots_of(case))
        for name, want in slotsr.items():
            assert np.abs(want[ec.INSIDE]).max() > 0, name
            worst["slots"] = max(worst["slots"], ec.bound_ratio(slots[name], want, ec.SLOT_RTOL, ec.slot_atol(want)))
        if avg is not None:
            worst["avg"] = max(worst["avg"], ec.bound_ratio(avg, avgr, ec.SLOT_RTOL, ec.slot_atol(avgr)))
        steps += 1
    assert steps == case.steps
    assert np.abs(pr - ec.start("p"))[ec.INSIDE].max() > 1e-4              # the case moved something
    _WORST[case.label] = worst
    return worst


@pytest.mark.parametrize("case", ec.CASES, ids=[c.label for c in ec.CASES])
def test_float32_restatement_stays_within_a_quarter_of_the_bound(case):
    """the device's arithmetic in numpy (optim_edge_cases.Float32Optimizer) against the float64 oracle, after every step, as ratios of
    tests/test_optim_gpu.py's bounds (parameters rtol 1e-5 + atol 1e-6; slots and the averaging slot rtol 1e-5 + atol 1e-6 max|slot|).
    The table's largest ratios are recorded in DESIGN.md, section 13."""
    worst = _worst_ratios(case)
    print("%s: worst error / bound  params %.3g  slots %.3g  avg %.3g" % (case.label, worst["params"], worst["slots"], worst["avg"]))
    assert max(worst.values()) <= ec.FLOAT32_CAP, worst


def test_float32_restatement_worst_ratios_per_kind():
    for kind in ec.KINDS:
        rows = [_worst_ratios(c) for c in ec.CASES if c.kind == kind]
        print("%s: worst error / bound  params %.3g  slots %.3g  avg %.3g" % (kind, max(r["params"] for r in rows),
                                                                              max(r["slots"] for r in rows), max(r["avg"] for r in rows)))
        assert max(max(r.values()) for r in rows) <= ec.FLOAT32_CAP


def test_huge_entries_give_a_finite_clipped_update():
    """1e20 entries: the oracle's norm is finite (sqrt(5) 1e20), so the segment is clipped to norm 1 -- a float32 sum of squares would be
    inf and, by the inf rule, zero the segment instead"""
    for label in ("sgd-var-huge", "adam-global-huge"):
        c = ec.CASE[label]
        o, n = ec.SEGMENTS[ec.HUGE_SEGMENT]
        ref = ec._make(RefOptimizer, c)
        g = ref.transform(np.where(ec.INSIDE, ec.gradients(c)[0], 0.0), ec.SEGMENTS)
        assert np.isfinite(g).all()
        np.testing.assert_allclose(np.abs(g[o:o + n]), 1.0 / np.sqrt(n), rtol=1e-12)      # the rest of the table is 1e-39 of the norm
        if c.norm == "global":
            np.testing.assert_allclose(np.sqrt(np.sum(g * g)), 1.0, rtol=1e-12)


# ---- the oracle's non-finite rules, by hand, on the 3-float and the 5-float segment --------------------------------------------
SEG3, SEG5 = (0, 3), (4, 5)


def _sgd_step(g, **clip):
    """one plain SGD step with lr 1 from p = 0: -p is the transformed gradient"""
    assert ec.SIZES[2] == SEG3[1] and ec.SIZES[3] == SEG5[1]
    p = np.zeros(9)
    RefOptimizer("sgd", 1.0, **clip).step(p, np.asarray(g, np.float64), [SEG3, SEG5])
    return -p


def test_oracle_inf_in_a_tail_zeroes_the_finite_entries_of_that_segment_only():
    #          3-float segment      pad   5-float segment: norm sqrt(1 + 4 + 4 + 16 + 0) = 5 -> g / 5
    d = _sgd_step([3.0, 4.0, np.inf, 0.0, 1.0, 2.0, 2.0, 4.0, 0.0], clipnorm=1.0)
    assert d[0] == 0.0 and d[1] == 0.0 and np.isnan(d[2])                   # finite * 1 / inf = 0, inf / inf = NaN
    np.testing.assert_allclose(d[4:], [0.2, 0.4, 0.4, 0.8, 0.0], rtol=1e-14)
    assert d[3] == 0.0
    d = _sgd_step([3.0, 4.0, 0.0, 0.0, 1.0, 2.0, 2.0, 4.0, -np.inf], clipnorm=1.0)
    np.testing.assert_allclose(d[:3], [0.6, 0.8, 0.0], rtol=1e-14)
    assert (d[4:8] == 0.0).all() and np.isnan(d[8])


def test_oracle_nan_in_a_tail_poisons_that_segment_only():
    d = _sgd_step([3.0, 4.0, 0.0, 0.0, 1.0, 2.0, 2.0, 4.0, np.nan], clipnorm=1.0)
    np.testing.assert_allclose(d[:3], [0.6, 0.8, 0.0], rtol=1e-14)
    assert np.isnan(d[4:]).all()
    d = _sgd_step([3.0, 4.0, np.nan, 0.0, 1.0, 2.0, 2.0, 4.0, 0.0], clipnorm=1.0)
    assert np.isnan(d[:3]).all()
    np.testing.assert_allclose(d[4:], [0.2, 0.4, 0.4, 0.8, 0.0], rtol=1e-14)


def test_oracle_non_finite_global_norm_poisons_everything_inside():
    for bad in (np.inf, np.nan):
        d = _sgd_step([3.0, 4.0, bad, 0.0, 1.0, 2.0, 2.0, 4.0, 0.0], global_clipnorm=1.0)
        assert np.isnan(d[:3]).all() and np.isnan(d[4:]).all() and d[3] == 0.0          # the padding is in no segment


def test_oracle_zero_norm_and_huge_entries_by_hand():
    d = _sgd_step([0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 2.0, 4.0, 0.0], clipnorm=1.0)
    assert (d[:3] == 0.0).all() and np.isfinite(d).all()                    # 0 * 1 / max(0, 1): no 0 / 0
    # norm of four 1e20 is 2e20: each becomes 1 / 2; the 3-float segment (norm 5 > 1) is clipped on its own
    d = _sgd_step([3.0, 4.0, 0.0, 0.0, 1e20, -1e20, 1e20, 1e20, 0.0], clipnorm=1.0)
    np.testing.assert_allclose(d, [0.6, 0.8, 0.0, 0.0, 0.5, -0.5, 0.5, 0.5, 0.0], rtol=1e-14)
    # global: N = sqrt(25 + 4e40) = 2e20 to 1e-39: everything is divided by it
    d = _sgd_step([3.0, 4.0, 0.0, 0.0, 1e20, -1e20, 1e20, 1e20, 0.0], global_clipnorm=1.0)
    np.testing.assert_allclose(d, [1.5e-20, 2e-20, 0.0, 0.0, 0.5, -0.5, 0.5, 0.5, 0.0], rtol=1e-14)
