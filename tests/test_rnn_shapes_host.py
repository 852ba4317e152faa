"""The case table of tests/test_rnn_shapes_gpu.py is worth running -- checked on the oracle alone, no device involved: the restated
launch arithmetic gives the values read off csrc/kws_rnn_kernels.h, the table reaches every template and branch for both kinds, the float64
oracle's gradients are finite and do not vanish, and the oracle restated in float32 lies at least rnn_cases.HOST_MARGIN times inside
every tolerance the device is held to, the per-row one included (so the tolerances are not set by the code under test)."""
import numpy as np
import pytest

import rnn_cases as rc

IDS = [c.label for c in rc.CASES]


def test_restated_launch_arithmetic():
    assert rc.gru_xstride(30, 20) == 626
    assert rc.gru_xstride(34, 20) == 690 and rc.gru_xstride(109, 20) == 2194 and rc.gru_xstride(54, 40) == 2162
    assert rc.gru_xstride(34, 64) == 2194 and rc.gru_xstride(110, 20) == 2226 and rc.gru_xstride(113, 20) == 2290
    assert all(rc.gru_xstride(T, F) % 32 == 18 and 0 <= rc.gru_xstride(T, F) - T * F < 32 for T in range(1, 120) for F in range(1, 65))
    # forward: 16 XS + 2 * 16 * 50 + 4 * 16 * 50 floats; at 23 x 40 XS = 946.  (16 * 946 + 4800) * 4 = 79,744: the tile of
    # test_other_geometries_train_and_infer's LSTM case, the only one above 64 KiB before this table
    assert rc.gru_xstride(23, 40) == 946 and rc.gru_fwd_smem(23, 40) == 79744
    # backward: 16 XS + 16 * 210 + 3 * 16 * 50 floats
    assert rc.gru_bwd_smem(109, 20) == 163456 <= rc.LDS_LIMIT == 163840
    # the limits in floats per clip: XS <= 2260 forward, XS <= 2200 backward
    assert (rc.LDS_LIMIT // 4 - 4800) // 16 == 2260 and (rc.LDS_LIMIT // 4 - 5760) // 16 == 2200
    assert rc.gru_fwd_smem(113, 20) == 4 * (16 * 2290 + 4800) > rc.LDS_LIMIT >= rc.gru_fwd_smem(110, 20) == 4 * (16 * 2226 + 4800)
    assert [rc.kx_for(F) for F in (1, 20, 21, 40, 41, 64)] == [5, 5, 10, 10, 16, 16]
    assert rc.head_bwd_fuses(2) and rc.head_bwd_fuses(48) and not rc.head_bwd_fuses(49)
    # the refusals of the GPU test: nothing fits at 113 x 20, only the forward tile at 110 x 20, and 109 x 20 is the last that trains
    assert not rc.infer_supported(*rc.REFUSED_INFER)
    assert rc.infer_supported(*rc.REFUSED_TRAIN) and not rc.train_supported(*rc.REFUSED_TRAIN)
    assert rc.train_supported(109, 20) and not rc.train_supported(65, 65)


def test_table_covers_every_template_and_branch():
    assert len(IDS) == len(set(IDS)) == 54
    for kind in rc.KINDS:
        cases = [c for c in rc.CASES if c.kind == kind]
        assert {rc.branch(c) for c in cases} == rc.REQUIRED_BRANCHES, kind
        assert all(rc.train_supported(c.T, c.F) for c in cases)
        by = lambda T, B, C=6: {c.F for c in cases if (c.T, c.B, c.C) == (T, B, C)}
        assert by(9, 21) == {1, 3, 20, 21, 37, 40, 41, 63, 64}
        assert {(c.T, c.F) for c in cases if c.label.split("-")[1].startswith("lds")} == {(30, 20), (34, 20), (40, 20), (109, 20), (54, 40), (34, 64)}
        assert all(c.B == 17 for c in cases if "-lds" in c.label or "-steps" in c.label)
        assert {c.T for c in cases if "-steps" in c.label} == {1, 2}
        assert {c.B for c in cases if (c.T, c.F, c.C) == (30, 20, 6)} >= {1, 15, 17, 100}
        assert {c.C for c in cases if (c.T, c.F, c.B) == (30, 20, 17)} == {2, 6, 48, 49}
        assert sum(c.class_weights is not None for c in cases) == 1
        assert sorted(c.dropout_seed for c in cases if "-seed" in c.label) == [0, rc.WIDE_SEED] and rc.WIDE_SEED >> 32
        # the only sequence at which the opt-in differs between the two kernels, and the longest each template trains
        assert rc.branch(rc.CASE[kind[7:] + "-lds34x20"])[1:3] == (False, True)
        for T, F in ((109, 20), (54, 40), (34, 64)):
            assert rc.train_supported(T, F) and not rc.train_supported(T + 1, F)


def _check_reference(case, ref):
    assert np.isfinite(ref.infer_probs).all() and np.isfinite(ref.probs).all() and np.isfinite(ref.loss)
    assert ref.infer_probs.shape == ref.probs.shape == (case.B, case.C)
    # no clip has its two best classes within twice the probability tolerance: the arg-max and the count of correct predictions are
    # then decided by anything that meets the tolerance, and the GPU test may ask for them exactly
    for p in (ref.infer_probs, ref.probs):
        top2 = np.sort(p, axis=-1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0]).min() > 2 * rc.PROB_ATOL, (case.label, (top2[:, 1] - top2[:, 0]).min())
    u = 144 if case.kind == "simple_gru" else 192
    assert ref.grads[0].shape == (case.F, u) and ref.grads[1].shape == (48, u)
    for name, g in zip(ref.names, ref.grads):
        assert np.isfinite(g).all(), name
        if case.T == 1 and name == "0/recurrent_kernel":
            assert not g.any()                          # h_prev is the zero initial state: exactly zero, not merely small
        else:
            assert np.abs(g).max() > 1e-4, (name, np.abs(g).max())


def _check_float32(case, saturated=False):
    ref = rc.reference(case, saturated)
    r32 = rc.run_oracle(case, np.float32, saturated)
    assert all(g.dtype == np.float32 for g in r32.grads) and r32.probs.dtype == np.float32
    fig, bad = rc.compare(ref, r32.infer_probs, r32.probs, r32.loss, r32.correct, r32.grads, margin=rc.HOST_MARGIN)
    print(case.label, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert not bad, bad
    return fig


@pytest.mark.parametrize("case", rc.CASES, ids=IDS)
def test_oracle_is_finite_and_float32_is_well_inside_the_tolerances(case):
    _check_reference(case, rc.reference(case))
    _check_float32(case)


@pytest.mark.parametrize("kind", rc.KINDS)
def test_shrinking_batch_and_saturated_cases_on_the_oracle(kind):
    for case in (rc.shrink_first_case(kind), rc.shrink_case(kind), rc.refused_train_case(kind)):
        _check_reference(case, rc.reference(case))
        _check_float32(case)
    case = rc.saturated_case(kind)
    ref = rc.reference(case, True)
    _check_reference(case, ref)
    _check_float32(case, True)
    # the bias puts the gates where it says: over the training pass a third of the units at exactly 1 in float32, a third at exactly 0
    om = rc.oracle_model(case, np.float32, True)
    x = rc.inputs(case)[0]
    with np.errstate(over="ignore"):
        om.logits(x, training=True)
    steps = om.layers[0].cache[2]
    gates = (1,) if kind == "simple_gru" else (3, 5)     # z of (h, z, r, hh, mh_h); f and o of (h, c, i, f, g, o, tc)
    for st in steps:
        for g in gates:
            assert (st[g][:, :16] == 1).all() and (st[g][:, 16:32] == 0).all()
            assert ((st[g][:, 32:] > 0) & (st[g][:, 32:] < 1)).all()
