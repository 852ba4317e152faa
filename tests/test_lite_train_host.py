"""The case table of tests/test_lite_train_gpu.py is sound -- checked on the host alone, no device involved: every stated grid, tile
count and padding follows from the restated launch arithmetic and the table reaches every branch of REQUIRED; the inputs meet the
condition under which a float32 implementation can be held to the device's bounds (tests/lite_train_cases.py, module docstring); and the
comparison can see what it is for -- an oracle that pads on the other side, or that loses the last block of a capped reduction, is
off by many tolerances."""
import numpy as np
import pytest

import cnn_path_cases as pc
import lite_train_cases as tc

IDS = [c.label for c in tc.CASES]


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def test_stated_values_follow_from_the_restated_arithmetic():
    assert len(set(IDS)) == len(IDS)
    for c in tc.CASES:
        M = tc.stage_rows(c.B, c.nf, c.fs)
        d = tc.dims(c.nf, c.fs)
        assert M == (c.B * c.nf * c.fs, c.B * d["H1"] * d["W1"], c.B * d["H3"] * d["W3"], c.B * d["H3"] * d["W3"]), c.label
        assert d["H4"] >= 1 and d["W4"] >= 1, c.label
        assert tc.stat_grid(M[0], 16) == c.stat1 and tc.stat_grid(M[1], 32) == c.stat2, c.label
        assert tc.dgrad_mw(M[1], tc.MI355X_CUS) == c.mw2 == pc.dgrad_mw([M[1]], 4 * tc.MI355X_CUS), c.label
        assert tc.pad3(c.nf, c.fs) == c.pad3 and tc.pool_drops(c.nf, c.fs) == c.drops and M[2] == c.m3, c.label
    by = tc.CASE
    # the caps: 8 R = 128 rows per block in stage 1, 64 in stage 2, and more once 1024 blocks no longer cover M
    assert [B for B in range(1, 600) if tc.stat_capped(600 * B, 16)][0] == 219
    assert [B for B in range(1, 600) if tc.stat_capped(150 * B, 32)][0] == 437
    assert by["under"].stat1[1] == 128 and by["cap1"].stat1 == (1019, 129) and by["cap2"].stat2[1] == 65 and by["under2"].stat2[1] == 64
    for c in tc.CASES:                                           # no other reduction of any case is capped (module docstring: out of scope)
        grids = tc.step_stat_grids(c.B, c.nf, c.fs)
        assert grids[0][1] == 16 and grids[2][1] == 32 and not any(tc.stat_capped(M, C) for M, C in grids[1:2] + grids[3:]), c.label
    # MW of conv_dgrad<32,16> on 256 compute units: 2 from 110 clips, 3 from 219, 4 from 328, 1 again at 437
    mw = [tc.dgrad_mw(150 * B, tc.MI355X_CUS) for B in range(0, 438)]
    assert set(mw[1:110]) == {1} and set(mw[110:219]) == {2} and set(mw[219:328]) == {3} and set(mw[328:437]) == {4} and mw[437] == 1
    # the small cases: less than one 16-row tile, and a 1 x 1 Dense kernel on the smallest map
    assert (by["b1"].m3, by["b2"].m3, by["b3"].m3, by["small1"].m3, by["small5"].m3) == (12, 24, 36, 4, 20)
    assert tc.dims(16, 16)["H4"] == tc.dims(16, 16)["W4"] == 1 and tc.stat_grid(1, 128) == (1, 1)
    # shrink: the second step's reductions use fewer blocks than the first's left behind
    sh = by["shrink"]
    for (M1, C1), (M2, C2) in zip(tc.step_stat_grids(sh.B, sh.nf, sh.fs), tc.step_stat_grids(sh.then, sh.nf, sh.fs)):
        assert C1 == C2 and tc.stat_grid(M2, C2)[0] < tc.stat_grid(M1, C1)[0]


def test_table_reaches_every_required_branch():
    got = set()
    for c in tc.CASES:
        for B in tc.batches(c):
            got |= tc.branches(B, c.nf, c.fs)
    assert tc.REQUIRED <= got, tc.REQUIRED - got
    # and with the issue's own rows alone everything but the stage-2 control
    issue = set().union(*(tc.branches(c.B, c.nf, c.fs) for c in tc.CASES if c.label != "under2"))
    assert tc.REQUIRED - issue == {"control2"}
    assert "cap1" not in tc.branches(218, 30, 20) and "cap1" in tc.branches(219, 30, 20)
    assert set(tc.DETERMINISTIC) <= set(IDS)


def test_stat_grid_covers_every_row_within_the_cap():
    seen = set()
    for c in tc.CASES:
        for B in tc.batches(c):
            seen |= set(tc.step_stat_grids(B, c.nf, c.fs))
    seen |= {(600 * B, 16) for B in range(1, 700, 7)} | {(M, 128) for M in range(1, 40)}
    for M, C in sorted(seen):
        nblk, rows = tc.stat_grid(M, C)
        assert 1 <= nblk <= tc.STAT_STRIDE and nblk * rows >= M > (nblk - 1) * rows, (M, C, nblk, rows)
        assert tc.stat_capped(M, C) == (rows > 8 * (256 // C)), (M, C, rows)


# ---- the condition on the inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=IDS)
def test_inputs_meet_the_condition(case):
    """a plain float32 implementation (oracle/torch_ref.py) stays within a third of the device's gradient bound, and no hard decision of
    the oracle's pass sits within TIE_MARGIN of its threshold.  This is a condition on the inputs: where a seed breaks it, another seed
    is chosen from these figures alone."""
    ref = tc.reference(case)
    assert all(w.dtype == np.float32 for w in ref.weights0) and len(ref.steps) == len(tc.batches(case))
    assert ref.zero_grad == ["0/bias", "4/bias"]
    for st in ref.steps:
        assert st.x.dtype == np.float32 and st.x.shape == (st.B, case.nf, case.fs) and np.isfinite(st.probs).all()
        assert st.margin >= tc.TIE_MARGIN, "pick another seed for %s: a decision %.1e from its threshold" % (case.label, st.margin)
    for threads in tc.RESTATEMENT_THREADS:
        for st, grads in zip(ref.steps, tc.restatement_grads(case, threads=threads)):
            figs = tc.grad_figures(ref, st, grads, tc.COND_REL, tc.ZERO_FLOOR)
            worst = tc.worst_gradient(figs)
            print("CONDITION | %s | B = %d | %d threads | restatement %.1e (%s) | zero-gradient biases %.1e | nearest decision %.1e" % (
                case.label, st.B, threads, worst.rel, worst.name, max(f.err for f in figs if f.rel != f.rel), st.margin))
            assert not tc.failures(figs), "pick another seed for %s: %s" % (case.label, tc.failures(figs))
        if case.label == "cap2":
            # the reason for SCALE: with the unscaled MFCC-like features the same restatement misses the condition at this batch
            full = tc.reference(case, 1.0)
            figs = tc.grad_figures(full, full.steps[0], tc.restatement_grads(case, 1.0, threads)[0], tc.COND_REL, tc.ZERO_FLOOR)
            print("CONDITION | cap2 unscaled | %d threads | restatement %.1e (%s)" % (threads, tc.worst_gradient(figs).rel, tc.worst_gradient(figs).name))
            assert tc.failures(figs)


# ---- the tests can fail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["pad01", "pad10"])
def test_a_swapped_padding_side_shows_in_depthwise_3(label):
    want, swapped = tc.swapped_padding_dw3_grad(tc.CASE[label])
    moved = float(np.abs(swapped - want).max() / np.abs(want).max())
    print("%s: padding on the other side moves 8/depthwise_kernel's gradient by %.3g of its largest entry" % (label, moved))
    assert moved > tc.PAD_MUTATION * tc.GRAD_REL, (label, moved)
    # and the oracle is back to TF's rule
    assert tc.mo.same_pad(6, 3, 2) == (3, 0, 1)


def test_a_dropped_last_block_shows_in_gamma_1():
    case = tc.CASE["cap1"]
    nblk, rows = case.stat1
    assert (nblk - 1) * rows == 1018 * 129 < 600 * case.B
    full, short = tc.truncated_gamma1_grad(case, (nblk - 1) * rows)
    moved = float(np.abs(short - full).max() / np.abs(full).max())
    print("cap1: without the last block 1/gamma's gradient moves by %.3g of its largest entry" % moved)
    assert moved > tc.CAP_MUTATION * tc.GRAD_REL, moved
