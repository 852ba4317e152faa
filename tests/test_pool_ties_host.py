"""The cases of tests/test_pool_ties_gpu.py tie where they are meant to, and a wrong routing rule at any pool shows in them -- checked
on the float64 oracle alone, no device involved.

Per scenario (tests/pool_tie_cases.py: a model kind, a map, a class count and a batch; its modes share one oracle pass) the tests
print the tie counts per pool, the per-tensor tolerance and the smallest movement over all (pool, rule) pairs.

The realistic scenario (glorot weights, clips that start with digital silence) ties between elements with identical patches only.
Routing to the last maximum cannot show there, and neither can the even split: it hands the same total to elements whose patches,
normalised values and gates are identical, so every weight, gamma and beta gradient keeps its value (measured: 7e-11 of a tolerance).
The one rule that case can catch is the one that gives every maximum the whole gradient, and that is what is asserted of it, at
pools 1 and 2; its third pool holds no tie."""
import numpy as np
import pytest

import pool_tie_cases as pt

IDS = [c.id.rsplit("-", 1)[0] for c in pt.SCENARIOS]


def pools_that_tie(case):
    return (0, 1) if case.realistic else (0, 1, 2)


def test_the_table_is_the_planned_one():
    ids = [c.id for c in pt.CASES]
    assert len(ids) == len(set(ids)) == 20
    by_kind = {k: sorted({(c.row.nf, c.row.fs) for c in pt.CASES if c.kind == k and not c.realistic}) for k in pt.KINDS}
    assert by_kind["simple_cnn"] == [(24, 16), (28, 20), (29, 13), (30, 20), (30, 22), (31, 21)]
    assert by_kind["simple_cnn_lite"] == [(24, 16), (29, 13), (30, 20)]
    modes = {}
    for c in pt.CASES:
        modes.setdefault((c.kind, c.row.name), []).append(c.mode)
        assert c.row.dropout_seed != 0 and c.row.C in (5, 49) and c.row.B in (5, 6, 17)
    assert modes[("simple_cnn", "map30x20")] == ["default", "fp32", "det", "fp32+det", "captured"]
    assert modes[("simple_cnn", "map28x20")] == ["default", "det"]
    assert modes[("simple_cnn", "map24x16")] == modes[("simple_cnn", "map29x13")] == ["default", "fp32"]
    assert modes[("simple_cnn_lite", "map30x20")] == ["default", "det"]
    assert [c.id for c in pt.CASES if c.realistic] == ["cnn-silence-default"]
    assert len(pt.SCENARIOS) == 12


def test_the_construction_is_exact():
    """every conv weight is zero off the centre tap and a signed power of two on it, one per output channel, every input channel read;
    the features are small integers"""
    for case in pt.SCENARIOS:
        if case.realistic:
            continue
        ref = pt.reference(case)
        om = ref.tao.om
        for l in om.layers:
            if isinstance(l, pt.mo.Conv2D):
                kernels = [l.kernel]
            elif isinstance(l, pt.mo.SeparableConv2D):
                kernels = [l.depthwise_kernel, l.pointwise_kernel]
                assert (l.bias * 8 == np.round(l.bias * 8)).all()
            else:
                continue
            for k in kernels:
                centre = k[k.shape[0] // 2, k.shape[1] // 2]
                assert np.abs(k).sum() == np.abs(centre).sum()
                nz = centre[centre != 0]
                assert set(np.abs(nz)) <= {1.0, 0.5, 0.25}
                if k.shape[3] == 1 and k.shape[2] > 1:                      # depthwise: one positive tap per channel
                    assert (centre > 0).all()
                else:
                    assert ((centre != 0).sum(0) == 1).all() and ((centre != 0).sum(1) >= 1).all()
        assert set(np.unique(ref.x)) <= {-2.0, -1.0, 0.0, 1.0}


def test_the_silent_frames_tie_bit_for_bit_in_the_oracle():
    """the realistic case rests on numpy's matrix product giving equal rows equal results: inside the silent frames of a clip the
    float64 oracle's first conv output repeats bit for bit from row to row and (off the c0 column's reach) from column to column"""
    case = [c for c in pt.SCENARIOS if c.realistic][0]
    ref = pt.reference(case)
    np.testing.assert_array_equal(ref.x[3, :12], np.broadcast_to(pt.silence_row(), (12, case.row.fs)))
    assert pt.silence_row()[0] < -30 and not pt.silence_row()[1:].any()
    z1 = ref.tao.om.layers[0].cache[2]
    for b in range(1, case.row.B):
        inner = z1[b, 1:4 * b - 1, 2:-1]              # rows whose 3 x 3 patch is silence only, columns that see neither c0 nor the edge
        assert inner.size and (inner == inner[:1, :1]).all(), b
    for p in (0, 1):
        assert pt.tie_stats(ref, p)["ties"] >= pt.MIN_TIES


@pytest.mark.parametrize("case", pt.SCENARIOS, ids=IDS)
def test_ties_exist_at_every_pool(case):
    ref = pt.reference(case)
    for p in pools_that_tie(case):
        s = pt.tie_stats(ref, p)
        print("TIES | %s | pool %d | %d of %d windows | horizontal %d vertical %d diagonal %d | first maximum not element 0: %d" % (
            IDS[pt.SCENARIOS.index(case)], p + 1, s["ties"], s["windows"], s["horizontal"], s["vertical"], s["diagonal"], s["first_not_0"]))
        assert s["ties"] >= pt.MIN_TIES, (p, s)
        if not case.realistic:
            assert s["horizontal"] >= 1 and s["vertical"] >= 1 and s["diagonal"] >= 1 and s["first_not_0"] >= 1, (p, s)


@pytest.mark.parametrize("case", pt.SCENARIOS, ids=IDS)
def test_no_decision_is_ambiguous(case):
    """no pool, ReLU6 or ReLU decision of the pass sits within 3e-6 of its threshold without sitting on it, and the ones that sit on
    it are exact on both sides"""
    ref = pt.reference(case)
    tao = ref.tao
    assert tao.n_near_ties == 0, "pick another seed: %s" % [c[:4] for c in tao.candidates]
    assert pt.unexplained_exact_decisions(case, ref) == []
    assert np.isfinite(tao.loss) and tao.probs.shape == (case.row.B, case.row.C)
    for w0, w1, t in zip(ref.weights0, ref.weights1, ref.trainable):
        assert t == np.array_equal(w0, w1)            # the pass moved every BatchNorm statistic: the device test asserts the same


@pytest.mark.parametrize("case", pt.SCENARIOS, ids=IDS)
def test_no_batchnorm_channel_sits_far_above_its_spread(case):
    """simple_cnn's split-precision path squares z in float32 for BatchNorm's variance: a channel with mean^2 far above var + eps (a
    constant one above all) would move the gradients by rounding alone (pool_tie_cases.MAX_MEAN2).  lite sums in double: printed only"""
    ref = pt.reference(case)
    ratios = pt.mean2_over_var(ref)
    print("MEAN2 | %s | largest mean^2 / (var + eps) per BatchNorm: %s | bound %.0f" % (
        IDS[pt.SCENARIOS.index(case)], " ".join("%.0f" % r for r in ratios), pt.MAX_MEAN2))
    if case.kind == "simple_cnn":
        assert max(ratios) <= pt.MAX_MEAN2, "pick another seed: %s" % ratios


@pytest.mark.parametrize("case", pt.SCENARIOS, ids=IDS)
def test_the_float32_oracle_picks_the_same_elements(case):
    ref = pt.reference(case)
    for li in ref.pools:
        np.testing.assert_array_equal(ref.arg32[li], ref.tao.om.layers[li].arg, err_msg="pool at layer %d" % li)


@pytest.mark.parametrize("case", pt.SCENARIOS, ids=IDS)
def test_every_alternative_rule_is_visible(case):
    """every (pool, alternative rule) moves some gradient tensor by at least 100 of that tensor's tolerances: a device that used the
    rule at that pool could not pass tests/test_pool_ties_gpu.py"""
    ref = pt.reference(case)
    name = IDS[pt.SCENARIOS.index(case)]
    print("TOL | %s | %s" % (name, " ".join("%s %.1e" % (n, t) for n, t in zip(ref.grad_names, ref.tol))))
    live = [t for t, z in zip(ref.tol, ref.zero) if not z]
    assert max(live) <= pt.MAX_TOL, "badly conditioned, pick another seed: %g" % max(live)
    assert min(live) >= pt.cc.grad_tol(case.row.B)
    moves = {(p, r): pt.movement(ref, p, r) for p in range(3) for r in pt.RULES}
    for (p, r), (m, tensor) in sorted(moves.items()):
        print("MOVES | %s | pool %d | %s | %.3g tolerances (%s)" % (name, p + 1, r, m, tensor))
    asserted = [(p, r) for p in pools_that_tie(case) for r in (pt.RULES if not case.realistic else ("every maximum",))]
    print("SMALLEST | %s | %.3g tolerances" % (name, min(moves[k][0] for k in asserted)))
    for k in asserted:
        assert moves[k][0] >= pt.VISIBLE, (k, moves[k])
    # the alternatives left the oracle with its baseline gradients
    assert all(np.array_equal(a, b) for a, b in zip(ref.tao.om.grad_list(), ref.tao.base))


def test_a_rule_moves_the_tensors_upstream_of_its_pool_only():
    """routing pool k differently leaves every tensor downstream of it untouched, and the failure message's pointer finds the pool:
    gradients made with one alternative are closest to that alternative"""
    case = pt.SCENARIOS[0]
    ref = pt.reference(case)
    for p, li in enumerate(ref.pools):
        alt = pt.alternative_grads(ref, p, "last maximum")
        moved = pt.grad_errors(ref, alt)
        for n, m in zip(ref.grad_names, moved):
            if int(n.split("/")[0]) > li:
                assert m == 0, (p, n, m)
        assert pt.closest_rule(ref, alt)[:2] == (p + 1, "last maximum")
    assert max(pt.grad_errors(ref, ref.tao.base)) == 0
