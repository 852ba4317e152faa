"""The case table of tests/test_quant_rnn_shapes_gpu.py is worth running -- checked on the numpy restatement alone
(tests/int8_rnn_ref.py), no device and no library involved: the table reaches every value of the F, T, C and B lists for both kinds,
the saturated GRU cases are saturated and bounded, no case is degenerate, the restatement's new hook leaves its results unchanged, and
the tolerances the device is held to (qrnn_cases.TOL) are the ones the restatement gives today."""
import numpy as np
import pytest

import int8_rnn_ref as ref
import qrnn_cases as qc

U = qc.U


def _ids(cases):
    return [c.label for c in cases]


def test_table_reaches_every_listed_value_for_both_kinds():
    labels = _ids(qc.EXACT_CASES + qc.TOLERANCE_CASES)
    assert len(labels) == len(set(labels))
    assert all(c.kind == "simple_gru" and c.weights == "saturated" for c in qc.EXACT_CASES)
    T0, F0, C0 = qc.BASE
    assert (T0, F0) != (30, 20)
    for cases in ([c for c in qc.EXACT_CASES if c.variant == "plain"],
                  [c for c in qc.TOLERANCE_CASES if c.kind == "simple_gru"], [c for c in qc.TOLERANCE_CASES if c.kind == "simple_lstm"]):
        full = [c for c in cases if c.B == c.N]
        assert {c.F for c in full if (c.T, c.C) == (T0, C0)} == {1, 15, 16, 17, 32, 33, 48, 49, 63, 64}
        assert {c.T for c in full if (c.F, c.C) == (F0, C0)} == {1, 2, 3, T0, 127, 128}
        assert {c.C for c in full if (c.T, c.F) == (T0, F0)} == {2, 15, 16, 17, 31, 32, 33, 47, 48}
        assert {(c.T, c.F, c.C) for c in full} >= {(1, 1, 2), (128, 64, 48), (127, 63, 47), (2, 17, 17)}
        part = [c for c in cases if c.B != c.N]
        assert sorted(c.B for c in part) == [1, 15, 16, 17, 33]
        assert all(c.start % 2 == 1 and c.start + c.B <= c.N and (c.T, c.F, c.C) == qc.BASE for c in part)
        assert {c.N for c in cases} == {qc.N_EXACT if cases[0].weights == "saturated" else qc.N_SHARE}
    assert {c.kind for c in qc.TOLERANCE_CASES} == set(qc.KINDS) and all(c.weights == "random" for c in qc.TOLERANCE_CASES)
    assert qc.N_EXACT == 3 * 16 + 1 and qc.N_SHARE == 16 * 16 + 1
    assert set(qc.TOL) == {c.array for c in qc.TOLERANCE_CASES}
    assert [c.variant for c in qc.EXACT_CASES if c.variant != "plain"] == list(qc.EXTRA_VARIANTS)


def test_builders_give_the_default_geometry_its_present_weights_and_features():
    """at F = 20, T = 30 the builders draw what tests/test_quant_rnn_gpu.py draws"""
    # that module is marked gpu but does no device work when imported (it imports torch inside its fixtures and tests): this host test
    # depends on it staying so
    import test_quant_rnn_gpu as old
    for a, b in zip(qc.saturated_gru(20, 11, 3), old._linear_gru(11, 3)):
        assert np.array_equal(a, b)
    for kind in qc.KINDS:
        for a, b in zip(qc.random_weights(kind, 20, 9, 21), old._random(kind, 9, 21)):
            assert np.array_equal(a, b)
    assert np.array_equal(qc.features(5, 30, 20, 4), old._features(5, 4))


@pytest.mark.parametrize("kind", qc.KINDS)
def test_the_hook_of_the_restatement_is_off_by_default_and_sees_every_gate(kind):
    """final_state with no hook, with a hook that returns what it is given and with a state list gives the same bits; the hook is
    called once per gate function and step; a perturbation of +-1e-6 moves the state a little and never by nothing"""
    T, F, C = 5, 9, 4
    ws = qc.random_weights(kind, F, C, 1)
    arr, x = ref.quantize(kind, ws), qc.features(6, T, F, 2)
    plain = ref.final_state(kind, arr, x)
    calls, states = [], []

    def hook(name, t, a, y):
        assert a.dtype == np.float32 and y.dtype == np.float64 and a.shape == y.shape == (6, U)
        calls.append((t, name))
        return y
    same = ref.final_state(kind, arr, x, hook, states)
    assert np.array_equal(plain.view(np.uint32), same.view(np.uint32))
    names = ["z", "r"] if kind == "simple_gru" else ["i", "f", "g", "o", "tc"]
    assert calls == [(t, n) for t in range(T) for n in names]
    assert len(states) == T and np.array_equal(states[-1], plain) and all(s.dtype == np.float32 for s in states)
    for k in range(1, T):                             # the states are those of the shorter sequences
        assert np.array_equal(states[k - 1], ref.final_state(kind, arr, x[:, :k]))
    moved = ref.final_state(kind, arr, x, ref.gate_noise(3))
    d = np.abs(moved.astype(np.float64) - plain).max()
    assert 0 < d < 1e-2
    again = ref.forward(kind, arr, x, ref.gate_noise(3))
    assert np.array_equal(again[0], ref.head(arr, moved)[0])
    assert np.array_equal(ref.forward(kind, arr, x)[0], ref.head(arr, plain)[0])


class _Trace(object):
    """the extremes of the saturated GRU's gate pre-activations"""

    def __init__(self):
        self.z_max, self.r_min = -np.inf, np.inf

    def __call__(self, name, t, a, y):
        if name == "z":
            self.z_max = max(self.z_max, float(a.max()))
            assert (y < 1e-34).all() and (1.0 - y == 1).all()        # e^-80 in float64: z h vanishes when h' is rounded to float32
        else:
            self.r_min = min(self.r_min, float(a.min()))
            assert (y == 1).all()
        return y


@pytest.mark.parametrize("case", [c for c in qc.EXACT_CASES if c.B == c.N], ids=lambda c: c.label)
def test_saturated_gru_cases_are_saturated_bounded_and_not_degenerate(case):
    ws = qc.weights(case)
    arr, x = ref.quantize(case.kind, ws), qc.feature_array(case)
    assert x.shape == (case.N, case.T, case.F) and x.dtype == np.float32 and np.isfinite(x).all()
    trace, states = _Trace(), []
    h = ref.final_state(case.kind, arr, x, trace, states)
    assert trace.z_max <= -80 and trace.r_min >= 80, (trace.z_max, trace.r_min)
    hmax = np.abs(np.stack(states)).max((0, 2))       # per clip, over steps and units
    assert np.isfinite(hmax).all()
    # a clip of the "spread" variant carries its factor: the recurrence is linear in x but for the biases
    allowed = 100.0 * np.maximum(1.0, qc.spread_factors(case)) if case.variant == "spread" else 100.0
    assert (hmax < allowed).all(), hmax.max()
    wl, wp, wa = qc.reference(case)
    assert np.array_equal(wl, ref.head(arr, h)[0])
    print(case.label, "max|h| %.3g  max|logit| %.3g" % (hmax.max(), np.abs(wl).max()))
    assert all(np.unique(wl[:, c]).size > case.N // 2 for c in range(case.C))          # the logits differ from clip to clip
    assert (qc.top2_gap(wl) > 0).all()                                                 # no exact tie: the arg-max is compared on every clip
    assert np.isfinite(wp).all() and np.abs(wp.sum(1, dtype=np.float64) - 1).max() < 1e-5
    if case.variant == "zeros":
        assert not x[:, qc.ZERO_STEP].any() and not x[qc.ZERO_CLIP].any() and np.count_nonzero(x[qc.SPARSE_CLIP]) == 1
        assert np.count_nonzero(x) > 0.9 * x.size * (case.T - 1) / case.T * (case.N - 2) / case.N
    if case.variant == "spread":
        f = qc.spread_factors(case)
        assert f.min() < 1e-2 and f.max() > 1e2 and np.unique(np.floor(np.log10(f[:16]))).size >= 4     # within one 16-clip wave too
    if case.variant == "zero_bias":
        assert not x[qc.ZERO_CLIP].any()
        assert all(not s[qc.ZERO_CLIP].any() for s in states)                           # h stays exactly 0 through all T steps
        assert np.array_equal(wl[qc.ZERO_CLIP], ws[4])                                  # the logits are the head bias
        assert all(s[np.arange(case.N) != qc.ZERO_CLIP].any(1).all() for s in states)


@pytest.mark.parametrize("case", [c for c in qc.TOLERANCE_CASES if c.B == c.N], ids=lambda c: c.label)
def test_recorded_tolerances_are_what_the_restatement_gives(case):
    devs = qc.noise_deviations(case)
    rec, tol = qc.TOL[case.array], qc.tolerance_figures(case, devs)
    print(case.label, "D %.4g  s %.4f  qerr %.4g  excluded %.4f  3D/qerr %.3f" % (tol.D, tol.s, tol.qerr, tol.excluded, 3 * tol.D / tol.qerr))
    assert tol.salt == rec.salt
    assert abs(tol.D - rec.D) <= 1e-5 * rec.D and abs(tol.qerr - rec.qerr) <= 1e-5 * rec.qerr, (tol, rec)
    assert abs(tol.s - rec.s) < 1e-4 and abs(tol.excluded - rec.excluded) < 1e-4, (tol, rec)
    assert rec.D > 0 and qc.DEVICE_FACTOR * rec.D < rec.qerr          # the case tells a correct kernel from an unquantized one
    assert rec.excluded <= qc.MAX_EXCLUDED                            # the arg-max rule leaves out at most 5 % of the clips
    assert 0 < rec.s <= 1
    wl = qc.reference(case)[0]
    assert rec.D > 10 * qc.tight_bound(case.T, wl).max()              # D holds at least one flipped code
    for part in (c for c in qc.TOLERANCE_CASES if c.array == case.array and c.B == 1):
        # the share rule asks the one clip of a B = 1 case to be inside the tight bound: it is, in every draw of the restatement
        assert (devs[:, part.start] <= qc.tight_bound(case.T, wl)[part.start]).all(), (part.label, devs[:, part.start])
        assert min(0.5, rec.s / 2) > 0
    assert np.isfinite(wl).all() and all(np.unique(wl[:, c]).size > case.N // 2 for c in range(case.C))
    # the rules the device is held to can be met: one more draw of the perturbed restatement meets them
    lg, _, am = ref.forward(case.kind, ref.quantize(case.kind, qc.weights(case)), qc.feature_array(case), ref.gate_noise(99991))
    fig, bad = qc.compare_tolerance(case, lg, am)
    assert not bad, (bad, fig)
    # ... and the unquantized model does not
    fl = ref.float_forward(case.kind, qc.weights(case), qc.feature_array(case))
    fig, bad = qc.compare_tolerance(case, fl, fl.argmax(1))
    assert bad and fig["worst"] == pytest.approx(rec.qerr, rel=1e-5)


@pytest.mark.parametrize("case", [c for c in qc.TOLERANCE_CASES if c.B != c.N], ids=lambda c: c.label)
def test_partial_batches_share_the_array_of_the_full_case(case):
    full = [c for c in qc.TOLERANCE_CASES if c.array == case.array and c.B == c.N]
    assert len(full) == 1 and full[0].N == case.N
    wl = qc.clips(case, qc.reference(case)[0])
    assert wl.shape == (case.B, case.C) and np.array_equal(wl, qc.reference(full[0])[0][1:1 + case.B])


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("C", qc.TIE_CLASSES)
def test_tied_head_columns_win_many_clips_on_the_restatement(kind, C):
    case = qc.head_case(kind, C, qc.N_SHARE, "tie")
    ws = qc.tied_weights(case)
    arr = ref.quantize(kind, ws)
    pairs = qc.tie_pairs(C)
    assert pairs == ((15, 16), (31, C - 1)) and all(i // 16 != j // 16 for i, j in pairs)
    lg, pr, am = ref.forward(kind, arr, qc.feature_array(case))
    for i, j in pairs:
        assert np.array_equal(arr["head_w"][:, i], arr["head_w"][:, j]) and arr["head_scale"][i] == arr["head_scale"][j]
        assert np.array_equal(lg[:, i], lg[:, j])
        wins = lg[:, i] == lg.max(1)
        assert wins.sum() >= 30, (i, j, wins.sum())   # the GPU test asks for 10 on the device
        assert (am[wins] == i).all()
    assert not np.isin(am, [j for _, j in pairs]).any()


@pytest.mark.parametrize("kind", qc.KINDS)
def test_underflow_head_leads_by_more_than_110_on_the_restatement(kind):
    case = qc.head_case(kind, qc.UNDERFLOW_C, qc.N_EXACT, "underflow")
    ws = qc.underflow_weights(case)
    lg, pr, am = ref.forward(kind, ref.quantize(kind, ws), qc.feature_array(case))
    lead = lg[:, -1].astype(np.float64) - lg[:, :-1].max(1)
    assert lead.min() > qc.UNDERFLOW_LEAD + 5         # the device's logits differ from these by far less (TOL)
    assert (am == case.C - 1).all() and (pr[:, -1] == 1).all() and not pr[:, :-1].any()
    assert np.float32(np.exp(np.float32(-qc.UNDERFLOW_LEAD))) == 0
    assert np.ptp(lg[:, :-1]) > 1                     # the other logits keep their spread
