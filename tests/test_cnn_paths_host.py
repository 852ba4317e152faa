"""The case table of tests/test_cnn_paths_gpu.py is sound -- checked on the float64 oracle alone, no device involved."""
import numpy as np
import pytest

import cnn_path_cases as cc


def test_case_ids_are_unique_and_the_table_is_what_the_modes_ask_for():
    ids = [c.id for c in cc.CASES]
    assert len(ids) == len(set(ids))
    assert len({r.name for r in cc.ROWS}) == len(cc.ROWS)
    assert len(cc.CASES) == 64
    by_mode = {m: [c.row.name for c in cc.CASES if c.mode == m] for m in cc.MODES}
    everything = [r.name for r in cc.ROWS]
    assert by_mode["fp32"] == by_mode["fp32+det"] == everything
    assert by_mode["det"] == [n for n in everything if not n.startswith("mw3")]
    assert by_mode["default"] == ["c49", "c100", "map29x13", "map40x24", "map24x16", "map62x21", "map28x20", "map30x22", "map31x21"]
    assert by_mode["captured"] == by_mode["captured+fp32"] == list(cc.CAPTURED_ROWS)
    for r in cc.ROWS:
        assert r.dropout_seed != 0 and r.B <= cc.MAX_ORACLE_BATCH
    # one weighted-loss variant per scenario, and one among the maps with the default tail
    assert [r.name for r in cc.ROWS if r.weighted] == ["b17", "c100", "map40x24", "map30x22"]


def test_restated_mw_rule_gives_the_intended_values():
    """launch_dgrad on a 256-CU part: conv3's data gradient is the first launch to leave MW = 1"""
    assert sorted(cc.MW_ROWS) == [1, 2, 3]
    for mw, (nf, fs, B) in cc.MW_ROWS.items():
        assert cc.dgrad_mws(B, nf, fs) == dict(conv3=mw, conv4=1, dense=1), (mw, B)
        r = cc.ROW[cc.mw_row_name(mw)]
        assert (r.nf, r.fs, r.B) == (nf, fs, B) and B <= cc.MAX_ORACLE_BATCH
    # the thresholds are the FIRST batch of each value on either map
    for (nf, fs), want in (((30, 20), {1: 1, 2: 468, 3: 937, 4: 1405}), ((62, 21), {1: 1, 2: 219, 3: 437, 4: 656})):
        firsts = {}
        for B in range(1, 1406):
            firsts.setdefault(cc.dgrad_mws(B, nf, fs)["conv3"], B)
        assert firsts == want, (nf, fs, firsts)
        assert cc.MW_BEYOND[4][(nf, fs)] == want[4] > cc.MAX_ORACLE_BATCH
    # every other row stays at MW = 1 in all three launches
    for r in cc.ROWS:
        if not r.name.startswith(("mw2", "mw3")):
            assert set(cc.dgrad_mws(r.B, r.nf, r.fs).values()) == {1}, r.name
    # the rule itself on hand-made inputs: one class of 16 * 1025 rows on 1024 SIMDs needs two rounds at MW = 1, one at MW = 2
    assert cc.dgrad_mw([16 * 1024], 1024) == 1 and cc.dgrad_mw([16 * 1025], 1024) == 2
    assert cc.dgrad_mw([16 * 2049], 1024) == 3 and cc.dgrad_mw([16 * 3073], 1024) == 4
    assert cc.parity_class_rows(2, 7, 5, 2) == [24, 16, 18, 12] and cc.parity_class_rows(3, 4, 3, 1) == [36]


@pytest.mark.parametrize("row", cc.ROWS, ids=[r.name for r in cc.ROWS])
def test_oracle_lists_few_enough_near_ties_to_enumerate(row):
    ref = cc.reference(row)
    tao = ref.tao
    assert tao.n_near_ties <= cc.MAX_CANDIDATES, "pick another feature seed for %s: %d near ties" % (row.name, tao.n_near_ties)
    assert len(tao.candidates) == tao.n_near_ties
    assert np.isfinite(tao.loss) and ref.infer_probs.shape == tao.probs.shape == (row.B, row.C)
    # the training pass moved the BatchNorm statistics (the device test asserts the same of the device's)
    for w0, w1, t in zip(ref.weights0, ref.weights1, ref.trainable):
        assert t == np.array_equal(w0, w1)
    # the inference argmax is asserted where the top-2 margin exceeds 1e-5: that must not be an empty set
    top2 = np.sort(ref.infer_probs, axis=-1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 1e-5).mean() > 0.9


def test_label_expectations_tell_the_paths_apart():
    """a case re-routed onto another mode's kernels must not satisfy its own expectation: the labels one mode requires hold one that
    the other mode forbids"""
    def clash(row, mode_a, mode_b):
        have_a, _ = cc.expected_labels(row, mode_a)
        _, lack_b = cc.expected_labels(row, mode_b)
        return [h for h in have_a for l in lack_b if l in h]
    for r in cc.ROWS:
        for mode in ("fp32", "det", "fp32+det"):
            assert clash(r, "default", mode), (r.name, mode)
            assert clash(r, mode, "default"), (r.name, mode)
        for a, b in (("fp32", "fp32+det"), ("det", "fp32+det"), ("det", "fp32")):
            assert clash(r, a, b) or clash(r, b, a), (r.name, a, b)
    have, lack = cc.expected_labels(cc.ROW["b65"], "fp32")
    assert "bf16" in lack and {"conv_wgrad<64,128>", "conv_dgrad<64,32>", "conv_gemm_fwd<32,64>"} <= set(have)
    have, lack = cc.expected_labels(cc.ROW["map29x13"], "default")
    assert not any("conv_group" in h for h in have) and "conv_group_fwd<32,64>" in lack
    # the maps with the default tail off the default map: the clip-group kernels with each of the plan's other switches both ways
    have, lack = cc.expected_labels(cc.ROW["map28x20"], "default")          # group, no fused pool, acc_bn2 without acc_fwd
    assert {"conv_group_fwd<32,64>", "bn_act_pool_kernel.L2", "bn_finalize_train_kernel.L2", "conv_wgrad_clip_bf16<16,32>",
            "l1_moments_kernel", "l1m_act_pool_kernel"} <= set(have)
    assert {"bn_bwd_finalize_kernel.L2", "bn_bwd_reduce_pool_kernel.L2", "l1_conv2_fwd_bf16<30,20>", "weight_split_kernel"} <= set(lack)
    have, lack = cc.expected_labels(cc.ROW["map30x22"], "default")          # group, no compact conv2 gradient, per-thread layer 1
    assert {"conv_group_fwd<32,64>", "conv_wgrad_clip<16,32>", "bn_bwd_reduce_pool_kernel.L2", "bn_bwd_finalize_kernel.L2",
            "l1_stats_kernel", "weight_split_kernel"} <= set(have)
    assert {"conv_wgrad_clip_bf16<16,32>", "l1_moments_kernel", "bn_bwd_finalize_kernel.L3"} <= set(lack)
    have, lack = cc.expected_labels(cc.ROW["map31x21"], "default")          # everything fused behind a per-thread layer 1
    assert {"conv_group_fwd<32,64>", "l1_stats_kernel", "l1_act_pool_kernel", "weight_split_kernel", "conv_fwd_clip_bf16<16,32>",
            "dense_head_fused_kernel"} <= set(have)
    assert {"bn_act_pool_kernel.L2", "bn_act_pool_kernel.L4", "bn_finalize_train_kernel.L2", "bn_bwd_finalize_kernel.L2",
            "l1_conv2_fwd_bf16<30,20>", "l1_moments_kernel"} <= set(lack)
    for name, s1 in (("map28x20", (14, 10)), ("map30x22", (15, 11)), ("map31x21", (15, 10))):
        d = cc.dims(cc.ROW[name].nf, cc.ROW[name].fs)
        assert (d["H1"], d["W1"]) == s1 and (d["H2"], d["W2"], d["H3"], d["W3"]) == (7, 5, 4, 3)
    # check_labels reports both kinds of complaint
    rep = dict.fromkeys(cc.expected_labels(cc.ROW["b65"], "default")[0])
    assert cc.check_labels(rep, cc.ROW["b65"], "default") == []
    assert cc.check_labels(rep, cc.ROW["b65"], "fp32")
