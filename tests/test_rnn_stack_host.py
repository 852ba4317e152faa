"""Host-side checks of the stacked recurrent models' reference and case table (tests/rnn_stack_ref.py, tests/rnn_stack_cases.py) and of
the host-only part of their interface (ModelSpec, KWSModel): no GPU."""
import numpy as np
import pytest

import rnn_cases as rc
import rnn_stack_cases as sc
import rnn_stack_ref as sr
from oracle import model_oracle as mo

TINY = dict(B=3, T=3, F=5, C=4)


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / (np.abs(want).max() + 1e-300))


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("weighted", (False, True))
def test_one_layer_reference_equals_the_oracle(kind, weighted):
    """num_layers = 1: logits, per-sample losses and every gradient equal oracle.model_oracle.Model's, with class weights and with a
    dropout seed (each <= 1e-12 of the quantity's largest entry)"""
    B, T, F, C, seed = 7, 6, 11, 5, 99173
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, T, F))
    y = rng.integers(0, C, B)
    cw = np.array(rc._weights(C)) if weighted else None
    m = sr.StackedModel(kind, C, T, F, 1).init_weights(3)
    om = mo.Model(kind, C, n_features=T, feature_size=F)
    om.set_weights(m.get_weights())
    om.set_dropout(seed, None)
    want_logits = om.logits(x, training=True)
    want_losses, dlogits = mo.loss_and_grad(mo.softmax(want_logits), y, cw)
    om.backward(dlogits)
    got_logits = m.logits(x, seed, training=True)
    got_losses = m.losses(x, y, cw, seed)[0]
    m.train_forward_backward(x, y, cw, seed)
    figures = {"logits": _rel(got_logits, want_logits), "losses": _rel(got_losses, want_losses)}
    for name, g, w in zip(m.names(), m.grad_list(), om.grad_list()):
        assert g.shape == w.shape and w.any()
        figures[name] = _rel(g, w)
    print(figures)
    assert max(figures.values()) <= 1e-12, figures
    assert _rel(m.predict(x), om.predict(x)) <= 1e-12


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("L", (2, 3))
def test_stacked_gradients_match_central_differences(kind, L):
    """the reference's BPTT against central finite differences of its own float64 loss, dropout on: relative error <= 1e-6 per tensor
    (of its largest entry), on 40 entries of every tensor drawn with a fixed seed -- all of them where the tensor has no more"""
    B, T, F, C = TINY["B"], TINY["T"], TINY["F"], TINY["C"]
    seed = 31337
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, T, F))
    y = rng.integers(0, C, B)
    m = sr.StackedModel(kind, C, T, F, L).init_weights(7)
    assert any((sr.layer_mask(seed, l, B, m.width(l)) == 0).any() for l in range(L)), "the seed drops nothing"
    m.train_forward_backward(x, y, None, seed)
    grads = [np.array(g) for g in m.grad_list()]
    ws = m.get_weights()
    eps = 1e-5

    def loss_at(ws_):
        m.set_weights(ws_)
        return float(m.losses(x, y, None, seed)[0].mean())
    for i, (name, g) in enumerate(zip(m.names(), grads)):
        num = np.array(g)
        for j in (range(g.size) if g.size <= 40 else np.random.default_rng(i).choice(g.size, 40, replace=False)):
            wp, wm = [w.copy() for w in ws], [w.copy() for w in ws]
            wp[i].flat[j] += eps
            wm[i].flat[j] -= eps
            num.flat[j] = (loss_at(wp) - loss_at(wm)) / (2 * eps)
        err = _rel(g, num)
        print(name, "%.2e" % err)
        assert err <= 1e-6, (name, err)


def test_layers_draw_different_masks():
    B, seed = 17, rc.WIDE_SEED
    masks = [sr.layer_mask(seed, l, B, sr.UNITS) for l in range(4)]
    for a in range(4):
        assert set(np.unique(masks[a])) == {0.0, 1.25}
        for b in range(a + 1, 4):
            assert (masks[a] != masks[b]).any()
    # layer 0 is the one-layer model's mask, seed 0 is no dropout anywhere
    np.testing.assert_array_equal(masks[0], mo.dropout_keep(seed, B * sr.UNITS, 0.2).reshape(B, sr.UNITS) / 0.8)
    assert sr.layer_seed(seed, 0) == seed and sr.layer_seed(2 ** 64 - 1, 1) == (sr.SEED_STEP - 1)
    assert all(sr.layer_mask(0, l, B, sr.UNITS) is None for l in range(4))


# ---- the host-only interface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("L", (1, 2, 4))
def test_model_spec_lays_out_every_layer_in_keras_order(kind, L):
    from kws_amd.model import ModelSpec
    F, C, T = 20, 6, 30
    spec = ModelSpec(kind, C, T, F, num_layers=L)
    ref = sr.StackedModel(kind, C, T, F, L)
    assert spec.num_layers == L
    assert [t["name"] for t in spec.tensors] == ref.names()
    assert [t["shape"] for t in spec.tensors] == [w.shape for w in ref.get_weights()]
    assert all(t["trainable"] for t in spec.tensors)
    offsets = [t["offset"] for t in spec.tensors]
    assert offsets == sorted(offsets) and offsets[0] == 0
    G = sr.GATES[kind]
    bias = 2 * 144 if kind == "simple_gru" else 192
    want = sum(G * 48 * ((F if l == 0 else 48) + 48) + bias for l in range(L)) + 48 * C + C
    assert spec.trainable_count() == want == sum(w.size for w in ref.get_weights())
    assert spec.workspace_bytes(4, True) > spec.workspace_bytes(4, False) > 0
    if L > 1:
        one = ModelSpec(kind, C, T, F)
        assert spec.workspace_bytes(4, False) > one.workspace_bytes(4, False)
        assert spec.workspace_bytes(4, True) > one.workspace_bytes(4, True)


def test_two_layer_gru_parameter_count():
    """F = 20, C = 6: 3*48*(20+48) + 288 = 10 080 for layer 0, 3*48*(48+48) + 288 = 14 112 for layer 1, 48*6 + 6 = 294 for the head"""
    from kws_amd.model import ModelSpec
    assert ModelSpec("simple_gru", 6, 30, 20, num_layers=2).trainable_count() == 10080 + 14112 + 294 == 24486


def test_one_layer_spec_is_the_unstacked_one():
    from kws_amd.model import ModelSpec
    for kind in rc.KINDS:
        a, b = ModelSpec(kind, 6, 30, 20), ModelSpec(kind, 6, 30, 20, num_layers=1)     # kws_model_create, kws_model_create_stacked(.., 1)
        assert a.num_layers == b.num_layers == 1
        assert a.tensors == b.tensors and a.param_count == b.param_count
        assert [a.workspace_bytes(33, t) for t in (False, True)] == [b.workspace_bytes(33, t) for t in (False, True)]


@pytest.mark.parametrize("kind,L", [("simple_gru", 0), ("simple_lstm", 0), ("simple_gru", 5), ("simple_lstm", 5), ("simple_cnn", 2),
                                    ("simple_cnn_lite", 2)])
def test_layer_counts_outside_the_range_are_refused(kind, L):
    from kws_amd import KwsError
    from kws_amd.model import ModelSpec
    with pytest.raises(KwsError, match="num_layers") as e:
        ModelSpec(kind, 6, 30, 20, num_layers=L)
    assert e.value.code == -1                       # KWS_ERR_INVALID


def test_host_quantizer_refuses_a_stacked_model():
    from kws_amd import KwsError
    from kws_amd.model import ModelSpec
    from kws_amd.quant import QuantizedRNN
    spec = ModelSpec("simple_gru", 6, 30, 20, num_layers=2)
    with pytest.raises(KwsError, match="num_layers") as e:
        QuantizedRNN.from_weights(spec, np.zeros((spec.param_count,), np.float32))
    assert e.value.code == rc.ERR_UNSUPPORTED


def test_kws_model_follows_num_layers(tmp_path):
    from classifier.model import KWSModel, get_model
    from classifier.params import pr
    m = KWSModel("simple_lstm", 5, seed=3, num_layers=3)
    assert [l["name"] for l in m.layers] == ["lstm_unit_0", "lstm_unit_1", "lstm_unit_2", "score_predict"]
    assert [l["output_shape"] for l in m.layers] == [(pr.n_features, 48), (pr.n_features, 48), (48,), (5,)]
    assert m.count_params() == sum(l["params"] for l in m.layers) == m.spec.trainable_count()
    lines = []
    m.summary(print_fn=lines.append)
    assert sum("(LSTM)" in s for s in lines) == 3
    ws = m.get_weights()
    assert len(ws) == 11
    for l in range(3):
        b = ws[3 * l + 2]
        assert (b[48:96] == 1).all() and not b[:48].any() and not b[96:].any()         # forget bias 1 in every layer
        u = ws[3 * l + 1][:, :48]
        np.testing.assert_allclose(u.T @ u, np.eye(48), atol=1e-5)                      # per-gate orthogonal
    for kind in ("simple_cnn", "simple_cnn_lite"):
        with pytest.raises(ValueError, match="num_layers"):
            KWSModel(kind, 5, num_layers=2)
    with pytest.raises(ValueError, match="num_layers"):
        KWSModel("simple_gru", 5, num_layers=5)
    # checkpoints: a one-layer file is what it was, a stacked one carries its layer count, and a mismatch names both counts
    one = KWSModel("simple_lstm", 5, seed=3)
    one.save_weights(str(tmp_path / "one.npz"))
    assert sorted(np.load(str(tmp_path / "one.npz")).files) == sorted(one.weight_names + ["__meta__", "__order__"])
    m.save_weights(str(tmp_path / "three.npz"))
    back = get_model("simple_lstm", 5, weights_path=str(tmp_path / "three.npz"), num_layers=3)
    for a, b in zip(back.get_weights(), ws):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match=r"num_layers = 3.*num_layers = 2"):
        get_model("simple_lstm", 5, weights_path=str(tmp_path / "three.npz"), num_layers=2)
    with pytest.raises(ValueError, match=r"num_layers = 1.*num_layers = 3"):
        m.load_weights(str(tmp_path / "one.npz"))
    one.load_weights(str(tmp_path / "one.npz"))


@pytest.mark.parametrize("tool", ("train", "eval", "listen"))
def test_command_line_tools_take_rnn_layers(tool):
    import importlib
    mod = importlib.import_module(tool)
    src = open(mod.__file__).read()
    assert "--rnn_layers" in src and "num_layers=" in src
    base = {"listen": ["--model_path", "x.npz", "--input_wav", "x.wav"], "train": ["--train_data_path", "x", "--classes_path", "y"],
            "eval": ["--weights_path", "x.npz", "--dataset_path", "x", "--classes_path", "y"]}[tool]
    assert mod.parse_args(base + ["--model_type", "simple_gru", "--rnn_layers", "2"]).rnn_layers == 2
    assert mod.parse_args(base + ["--model_type", "simple_gru"]).rnn_layers == 1
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--model_type", "simple_cnn", "--rnn_layers", "2"])


# ---- the case table -------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_branch():
    for kind in rc.KINDS:
        got = {sc.branch(c) for c in sc.CASES if c.kind == kind}
        assert sc.REQUIRED_BRANCHES <= got, sc.REQUIRED_BRANCHES - got
    labels = [c.label for c in sc.CASES]
    assert len(set(labels)) == len(labels)
    for c in sc.CASES:
        assert sc.infer_supported(c) and sc.train_supported(c), c.label
        assert c.L in (2, 3, 4)
    for kind in rc.KINDS:
        mine = [c for c in sc.CASES if c.kind == kind]
        assert {c.L for c in mine} == {2, 3, 4}
        assert {c.T for c in mine} >= {1, 2, 9, 14, 39, sc.LONGEST_TRAIN_T}
        assert {c.B for c in mine if (c.T, c.F) == (9, 20)} >= {1, 15, 17, 33}
        assert {c.F for c in mine} >= {3, 13, 20, 37, 64}
        assert {c.C for c in mine} == {6, 49}
        assert {c.dropout_seed for c in mine} >= {0, rc.WIDE_SEED}
        assert any(c.class_weights for c in mine)
        assert any((c.L, c.T, c.F, c.B) == (4, 5, 20, 17) for c in mine) and any((c.L, c.T, c.F) == (2, 39, 13) for c in mine)


def test_lds_edges_of_the_48_wide_layers():
    """the table in rnn_stack_cases' docstring, from the restated arithmetic"""
    assert rc.gru_xstride(45, 48) == 2162 and rc.gru_xstride(46, 48) == 2226
    assert rc.gru_bwd_smem(45, 48) == 161408 <= rc.LDS_LIMIT
    assert rc.gru_fwd_smem(46, 48) == 161664 <= rc.LDS_LIMIT < rc.gru_bwd_smem(46, 48) == 165504
    assert (rc.gru_fwd_smem(14, 48), rc.gru_bwd_smem(14, 48)) == (63360, 67200)
    assert (rc.gru_fwd_smem(9, 48), rc.gru_bwd_smem(9, 48)) == (46976, 50816)
    assert (rc.gru_fwd_smem(30, 48), rc.gru_bwd_smem(30, 48)) == (112512, 116352)
    for kind in rc.KINDS:
        c = sc.refused_train_case(kind)
        assert sc.infer_supported(c) and not sc.train_supported(c)
        assert rc.train_supported(c.T, c.F)             # layer 0 alone would train: the refusal comes from the layer above
        first, second = sc.shrink_cases(kind)
        assert (first.B, second.B) == rc.SHRINK and sc.train_supported(first)


def test_float32_reference_stays_a_tenth_inside_the_gpu_tolerances():
    """The GPU tolerances are rnn_cases' own for every tensor: the float32 run of the reference stays within a tenth of each on every GPU
    case.  Largest figures on this table when it was written: inference probabilities 2.6e-7 and training probabilities 5.9e-7 (bound
    1e-4), loss 1.0e-6 (1e-4), gradients 1.3e-6 of a tensor's largest entry (layer 0's kernel; 2e-4), worst row of layer 0's kernel
    1.3e-6."""
    worst = {}
    for c in sc.CASES + [sc.refused_train_case(k) for k in rc.KINDS] + [x for k in rc.KINDS for x in sc.shrink_cases(k)]:
        _, ref = sc.reference(c)
        r32 = sc.run_float32(c)
        fig, bad = rc.compare(ref, r32.infer_probs, r32.probs, r32.loss, r32.correct, r32.grads, margin=sc.FLOAT32_MARGIN)
        for k, v in fig.items():
            k = k.split(" (")[0]
            worst[k] = max(worst.get(k, 0.0), v)
        assert not bad, (c.label, bad)
    print({k: "%.2e" % v for k, v in worst.items()})
