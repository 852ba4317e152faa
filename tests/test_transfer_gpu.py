"""GPU tests of the transfer feature: kws_model_embed for every model kind, kws_head_fit (csrc/kws_transfer.hip) against the float64
reference of tests/transfer_ref.py at the cases of tests/transfer_cases.py, its determinism and the independence of its jobs, and what
kws_amd.transfer and train.py --freeze_backbone build on them."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import geometry_cases as gc
import rnn_stack_ref as sr
import transfer_cases as tc
import transfer_ref as tr
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu

OFF_DEFAULT = gc.ROW["tuned-14"]            # 14 frames x 20 coefficients


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def softmax64(z):
    return mo.softmax(np.asarray(z, np.float64))


# ---- embed ----------------------------------------------------------------------------------------------------------------------
def _oracle(kind, layers, C, nf, fs, seed, dtype):
    """-> (weights in Keras order, function x -> the activation in front of the last Dense) of an oracle with non-trivial statistics"""
    if layers > 1:
        om = sr.StackedModel(kind, C, nf, fs, layers).init_weights(seed)
        m = sr.StackedModel(kind, C, nf, fs, layers, dtype)
        m.set_weights(om.get_weights())

        def act(x):
            m.logits(x)
            return m.h_last
        return om.get_weights(), act
    om = mo.Model(kind, C, n_features=nf, feature_size=fs).init_weights(seed)
    rng = np.random.default_rng(seed + 1)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    m = mo.Model(kind, C, n_features=nf, feature_size=fs, dtype=dtype)
    m.set_weights(ws)

    def act(x):
        x = np.asarray(x, dtype)
        if m.input_rank == 4:
            x = x[..., None]
        for l in m.layers[:-1]:
            x = l.forward(x, False)
        return x
    return ws, act


EMBED_MODELS = [("simple_cnn", 1), ("simple_cnn_lite", 1), ("simple_gru", 1), ("simple_lstm", 1), ("simple_lstm", 2)]
_embed_cache = {}


def _embed_case(torch, kind, layers, nf, fs):
    """the oracle's activations at B = 17 (B = 1 is its first row), computed once per (model, map)"""
    key = (kind, layers, nf, fs)
    if key not in _embed_cache:
        C = 7
        rng = np.random.default_rng(nf * 31 + fs)
        x = (rng.standard_normal((17, nf, fs)) * 2.0).astype(np.float32)
        ws, act64 = _oracle(kind, layers, C, nf, fs, 5, np.float64)
        _, act32 = _oracle(kind, layers, C, nf, fs, 5, np.float32)
        _embed_cache[key] = dict(C=C, x=x, ws=ws, e64=act64(x), e32=act32(x))
    return _embed_cache[key]


@pytest.mark.parametrize("B", (1, 17))
@pytest.mark.parametrize("nf,fs", [(30, 20), (OFF_DEFAULT.frames, gc.feature_size(OFF_DEFAULT))])
@pytest.mark.parametrize("kind,layers", EMBED_MODELS)
def test_embed(torch, kind, layers, nf, fs, B):
    from kws_amd.model import DeviceModel, ModelSpec
    c = _embed_case(torch, kind, layers, nf, fs)
    dm = DeviceModel(ModelSpec(kind, c["C"], nf, fs, layers if layers > 1 else None))
    dm.set_weights(c["ws"])
    E = 128 if "cnn" in kind else 48
    assert dm.embed_size == E
    xt = torch.from_numpy(c["x"][:B]).cuda()
    ws = dm.new_workspace(B)
    dm.prepare_inference(B, ws)
    p0, a0 = dm.forward(xt, workspace=ws)
    emb = dm.embed(xt, workspace=ws)
    p1, a1 = dm.forward(xt, workspace=ws)
    assert emb.shape == (B, E) and emb.dtype == torch.float32
    e = emb.cpu().numpy()
    # (c) the prepared state of the workspace was dropped, not misread: the same probabilities before and after
    assert torch.equal(p0, p1) and torch.equal(a0, a1)
    # (a) the model's own head on the returned embeddings gives forward's probabilities
    head = softmax64(e.astype(np.float64) @ np.asarray(c["ws"][-2], np.float64) + np.asarray(c["ws"][-1], np.float64))
    err_a = float(np.abs(head - p0.cpu().numpy()).max())
    # (b) the oracle's activation in front of its last Dense; the tolerance from the same oracle in float32
    tol = max(4.0 * float(np.abs(c["e32"][:B].astype(np.float64) - c["e64"][:B]).max()), 1e-6)
    err_b = float(np.abs(e - c["e64"][:B]).max())
    print(kind, layers, (nf, fs), B, "head %.3g (1e-4)  oracle %.3g (tol %.3g)" % (err_a, err_b, tol))
    assert err_a <= 1e-4
    assert err_b <= tol
    if "cnn" in kind:
        assert e.min() >= 0.0 and e.max() <= 6.0            # behind ReLU6


def test_embed_ignores_the_inference_precision(torch):
    """(d) simple_cnn_lite at KWS_INFER_FP16: the same bits as without"""
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    c = _embed_case(torch, "simple_cnn_lite", 1, 30, 20)
    dm = DeviceModel(ModelSpec("simple_cnn_lite", c["C"], 30, 20))
    dm.set_weights(c["ws"])
    xt = torch.from_numpy(c["x"]).cuda()
    e0 = dm.embed(xt)
    dm.set_precision(infer=L.INFER_FP16)
    p16, _ = dm.forward(xt)
    e1 = dm.embed(xt)
    p16b, _ = dm.forward(xt)
    dm.set_precision(infer=None)
    p32, _ = dm.forward(xt)
    assert torch.equal(e0, e1)
    assert torch.equal(p16, p16b)
    assert not torch.equal(p16, p32)                        # the switch was on: the forward took the fp16 kernels


# ---- head fit against the reference ---------------------------------------------------------------------------------------------
def _split(flat, E, C):
    flat = flat.cpu().numpy()
    return flat[:E * C].reshape(E, C), flat[E * C:]


def _got(head):
    E, C = head.embed_size, head.num_classes
    mk, mb = _split(head.state["m"], E, C)
    vk, vb = _split(head.state["v"], E, C)
    return dict(kernel=head.kernel, bias=head.bias, m_kernel=mk, m_bias=mb, v_kernel=vk, v_bias=vb)


def _job(case, d, order=None, **kw):
    j = dict(order=d["order"] if order is None else order, num_classes=case.C, batch_size=case.batch, init=(d["kernel"], d["bias"]))
    j.update(tc.job_kw(case, d))
    j.update(kw)
    return j


@pytest.mark.parametrize("case", [c for c in tc.CASES if c.n_order > 0], ids=lambda c: c.name)
def test_head_fit_matches_the_reference(torch, case):
    from kws_amd import transfer as T
    d, ref, tol = tc.expected(case)
    head = T.fit_heads(torch.from_numpy(d["emb"]).cuda(), d["labels"], [_job(case, d)])[0]
    got = _got(head)
    got["loss_sum"], got["hits"] = head.loss[0] * case.n_order, head.accuracy[0] * case.n_order
    figures = {q: (float(np.abs(np.asarray(got[q], np.float64) - ref[q]).max()), tol[q]) for q in tc.QUANTITIES}
    print(case.name, {q: "%.3g (tol %.3g)" % f for q, f in figures.items()})
    for q, (err, t) in figures.items():
        assert err <= t, (case.name, q, err, t)
    steps = -(-case.n_order // case.batch)
    assert head.state["t"] == steps
    if case.name == "ignored-batch":
        assert float(np.abs(ref["kernel"] - d["kernel"]).max()) > steps * 0.5e-3      # every step moved the weights, the ignored one too


def _raw_launch(torch, emb, labels, order, jobs, W, M, V, stats, cw=None):
    from kws_amd import lib as L
    recs = (L.KwsHeadJob * len(jobs))(*jobs)
    jd = torch.empty((ctypes.sizeof(recs),), dtype=torch.uint8, device="cuda")
    L.check(L.get_lib().kws_head_fit(emb.data_ptr(), labels.data_ptr(), emb.shape[0], emb.shape[1], order.data_ptr(),
                                     cw.data_ptr() if cw is not None else None, recs, jd.data_ptr(), len(jobs), W.data_ptr(),
                                     M.data_ptr() if M is not None else None, V.data_ptr() if V is not None else None, stats.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def test_empty_job_changes_no_bit(torch):
    """n_order = 0: weights, slots and the job's stats keep every bit, next to a job of the same launch that does train"""
    from kws_amd import lib as L
    case = tc.CASE["base"]
    d = tc.data(case)
    n = (case.E + 1) * case.C
    rng = np.random.default_rng(0)
    W = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    M = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    V = torch.from_numpy(rng.uniform(0, 1, 2 * n).astype(np.float32)).cuda()
    stats = torch.full((2, 2), 7.0, dtype=torch.float32, device="cuda")
    before = [t.clone() for t in (W, M, V)]
    jobs = []
    for i, n_order in enumerate((0, 32)):
        j = L.KwsHeadJob()
        j.order_offset, j.weight_offset, j.class_weight_offset, j.t0 = 0, i * n, -1, 3
        j.n_order, j.batch, j.num_classes, j.ignore_index, j.optimizer = n_order, case.batch, case.C, 0, L.OPT_KINDS["adam"]
        j.lr, j.beta1, j.beta2, j.eps, j.momentum = 1e-3, 0.9, 0.999, 1e-7, 0.0
        jobs.append(j)
    _raw_launch(torch, torch.from_numpy(d["emb"]).cuda(), torch.from_numpy(d["labels"]).cuda(), torch.from_numpy(d["order"]).cuda(), jobs,
                W, M, V, stats)
    for t, b in zip((W, M, V), before):
        assert torch.equal(t[:n], b[:n])
        assert not torch.equal(t[n:], b[n:])
    assert stats[0].tolist() == [7.0, 7.0] and stats[1, 0].item() != 7.0


def test_null_slots_start_at_zero_and_are_not_stored(torch):
    from kws_amd import lib as L
    case = tc.CASE["steps2"]
    d, ref, tol = tc.expected(case)
    n = (case.E + 1) * case.C
    W = torch.from_numpy(np.concatenate([d["kernel"].reshape(-1), d["bias"]])).cuda()
    stats = torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    j = L.KwsHeadJob()
    j.order_offset, j.weight_offset, j.class_weight_offset, j.t0 = 0, 0, -1, 0
    j.n_order, j.batch, j.num_classes, j.ignore_index, j.optimizer = case.n_order, case.batch, case.C, 0, L.OPT_KINDS["adam"]
    j.lr, j.beta1, j.beta2, j.eps, j.momentum = case.lr, 0.9, 0.999, 1e-7, 0.0
    _raw_launch(torch, torch.from_numpy(d["emb"]).cuda(), torch.from_numpy(d["labels"]).cuda(), torch.from_numpy(d["order"]).cuda(), [j],
                W, None, None, stats)
    k, b = _split(W, case.E, case.C)
    assert float(np.abs(k - ref["kernel"]).max()) <= tol["kernel"] and float(np.abs(b - ref["bias"]).max()) <= tol["bias"]
    assert n == W.numel()


def test_continuing_equals_one_launch(torch):
    """8 steps, then 8 more from the carried state with t0 = 8: bit for bit the 16 steps of one launch"""
    from kws_amd import transfer as T
    case = tc._case("sixteen", steps=16, seed=31)
    d = tc.data(case)
    emb = torch.from_numpy(d["emb"]).cuda()
    one = T.fit_heads(emb, d["labels"], [_job(case, d)])[0]
    half = 8 * case.batch
    a = T.fit_heads(emb, d["labels"], [_job(case, d, order=d["order"][:half])])[0]
    assert a.state["t"] == 8
    b = T.fit_heads(emb, d["labels"], [_job(case, d, order=d["order"][half:], init=a, state=a.state)])[0]
    assert b.state["t"] == 16 == one.state["t"]
    assert torch.equal(one.weights, b.weights) and torch.equal(one.state["m"], b.state["m"]) and torch.equal(one.state["v"], b.state["v"])
    assert not torch.equal(a.weights, b.weights)
    # and the same for the momentum buffer of SGD
    sgd = dict(optimizer="sgd", lr=0.05, momentum=0.9)
    one = T.fit_heads(emb, d["labels"], [_job(case, d, **sgd)])[0]
    a = T.fit_heads(emb, d["labels"], [_job(case, d, order=d["order"][:half], **sgd)])[0]
    b = T.fit_heads(emb, d["labels"], [_job(case, d, order=d["order"][half:], init=a, state=a.state, **sgd)])[0]
    assert torch.equal(one.weights, b.weights) and torch.equal(one.state["m"], b.state["m"])


# ---- determinism and independence ---------------------------------------------------------------------------------------------------
def _three_jobs(rng, N):
    return [dict(order=rng.permutation(N)[:150].astype(np.int32), num_classes=5, batch_size=16, seed=1),
            dict(order=np.zeros((0,), np.int32), num_classes=17, batch_size=7, seed=2),
            dict(order=rng.integers(0, N, 77).astype(np.int32), num_classes=40, batch_size=33, seed=3, optimizer="sgd", lr=0.05, momentum=0.9)]


def _bits(h):
    return (h.weights, h.state["m"], h.state["v"])


def test_jobs_are_deterministic_and_independent(torch):
    from kws_amd import transfer as T
    rng = np.random.default_rng(41)
    N = 200
    emb = torch.from_numpy(tc.embeddings(rng, N, 128)).cuda()
    y = rng.integers(0, 5, N)
    jobs = _three_jobs(rng, N)
    first, second = T.fit_heads(emb, y, jobs), T.fit_heads(emb, y, jobs)
    for a, b in zip(first, second):
        assert all(torch.equal(p, q) for p, q in zip(_bits(a), _bits(b)))
        assert a.loss == b.loss or (np.isnan(a.loss[0]) and np.isnan(b.loss[0]))
    for job, a in zip(jobs, first):
        alone = T.fit_heads(emb, y, [job])[0]               # another instantiation of the kernel when the job is the narrow one
        assert all(torch.equal(p, q) for p, q in zip(_bits(a), _bits(alone)))
        assert a.loss == alone.loss or np.isnan(a.loss[0])
    # the empty job still holds its initial value
    k, b = T.glorot_head(128, 17, 2)
    np.testing.assert_array_equal(first[1].kernel, k)
    assert not first[1].bias.any() and first[1].state["t"] == 0
    assert not np.array_equal(first[0].kernel, T.glorot_head(128, 5, 1)[0])


def test_more_jobs_than_compute_units(torch):
    """J = 300 identical tiny jobs: 300 identical results"""
    from kws_amd import transfer as T
    rng = np.random.default_rng(43)
    N = 64
    emb = torch.from_numpy(tc.embeddings(rng, N, 48)).cuda()
    y = rng.integers(0, 3, N)
    job = dict(order=rng.permutation(N)[:40].astype(np.int32), num_classes=3, batch_size=16, seed=9)
    heads = T.fit_heads(emb, y, [job] * 300)
    assert len(heads) == 300
    for h in heads[1:]:
        assert all(torch.equal(p, q) for p, q in zip(_bits(h), _bits(heads[0])))
        assert h.loss == heads[0].loss and h.accuracy == heads[0].accuracy
    assert np.isfinite(heads[0].loss[0]) and not np.array_equal(heads[0].kernel, T.glorot_head(48, 3, 9)[0])


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
PY = dict(N=150, E=128, C=6, batch=32, epochs=3, lrs=[1e-3, 5e-4, 2.5e-4], seed=52)


def test_fit_head_epochs_and_schedule(torch):
    """3 epochs with a learning rate per epoch against the reference driven with the same seeded permutations; the tolerance rule and the
    summation-order check of tests/transfer_cases.py, applied to this configuration"""
    from kws_amd import transfer as T
    rng = np.random.default_rng(PY["seed"])
    emb = tc.embeddings(rng, PY["N"], PY["E"])
    y = rng.integers(0, PY["C"], PY["N"])
    orders = T.epoch_orders(np.arange(PY["N"]), PY["epochs"], PY["seed"])
    k0, b0 = T.glorot_head(PY["E"], PY["C"], PY["seed"])
    runs = {}
    for name, dtype, rev in (("ref64", np.float64, False), ("ref32", np.float32, False), ("rev32", np.float32, True)):
        runs[name] = tr.fit_head(emb, y, PY["C"], orders, PY["batch"], k0, b0, PY["lrs"], dtype=dtype, reverse=rev)
    head = T.fit_head(torch.from_numpy(emb).cuda(), y, PY["C"], epochs=PY["epochs"], batch_size=PY["batch"], lr=PY["lrs"], seed=PY["seed"])
    st64, loss64, acc64 = runs["ref64"]
    assert head.state["t"] == st64.t == PY["epochs"] * 5
    for q, got in (("kernel", head.kernel), ("bias", head.bias), ("loss", np.array(head.loss)), ("accuracy", np.array(head.accuracy))):
        pick = (lambda r: getattr(r[0], q)) if q in ("kernel", "bias") else (lambda r: np.array(r[1] if q == "loss" else r[2]))
        want = np.asarray(pick(runs["ref64"]), np.float64)
        tol = max(4.0 * float(np.abs(np.asarray(pick(runs["ref32"]), np.float64) - want).max()), 1e-6)
        assert float(np.abs(np.asarray(pick(runs["rev32"]), np.float64) - want).max()) <= tol, (q, "the seed is order sensitive")
        err = float(np.abs(np.asarray(got, np.float64) - want).max())
        print(q, "%.3g (tol %.3g)" % (err, tol))
        assert err <= tol, (q, err, tol)
    assert len(head.loss) == 3 and head.loss[2] < head.loss[0]


def _kws_model(kind, C, seed):
    from classifier.model import KWSModel
    m = KWSModel(kind, C, seed=seed)
    ws = m.get_weights()
    rng = np.random.default_rng(seed)
    for i, n in enumerate(m.weight_names):
        if n.endswith(("gamma", "moving_variance")):
            ws[i] = (ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)).astype(np.float32)
        elif n.endswith(("beta", "bias", "moving_mean")):
            ws[i] = (ws[i] + 0.1 * rng.standard_normal(ws[i].shape)).astype(np.float32)
    m.set_weights(ws)
    return m


@pytest.mark.parametrize("kind", ("simple_cnn", "simple_gru"))
def test_with_head(torch, kind, tmp_path):
    from classifier.model import KWSModel
    from classifier.params import pr
    from kws_amd import transfer as T
    model = _kws_model(kind, 12, 3)
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((40, pr.n_features, pr.feature_size)) * 2.0).astype(np.float32)
    y = rng.integers(0, 3, 40)
    emb = T.embed(model, x, batch_size=16)                  # three batches, the last one partial
    assert emb.shape == (40, model._device().embed_size)
    head = T.fit_head(emb, y, 3, epochs=2, batch_size=8, seed=1)
    new = T.with_head(model, head)
    assert new.num_classes == 3 and new.model_type == kind and model.num_classes == 12
    want = softmax64(emb.cpu().numpy().astype(np.float64) @ head.kernel.astype(np.float64) + head.bias.astype(np.float64))
    got = new.predict(x)
    assert got.shape == (40, 3)
    np.testing.assert_allclose(got, want, atol=1e-4, rtol=0)
    for a, b in zip(model.get_weights()[:-2], new.get_weights()[:-2]):
        np.testing.assert_array_equal(a, b)
    path = str(tmp_path / "tuned.npz")
    new.save_weights(path)
    back = KWSModel(kind, 3)
    back.load_weights(path)
    for a, b in zip(new.get_weights(), back.get_weights()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(back.predict(x), got)


def test_cross_validate_equals_separate_fits(torch):
    from kws_amd import transfer as T
    rng = np.random.default_rng(61)
    N, C = 90, 4
    centers = rng.uniform(-1, 1, (C, 48))
    y = rng.integers(0, C, N)
    emb = torch.from_numpy((centers[y] * 0.5 + 0.3 * rng.standard_normal((N, 48))).astype(np.float32)).cuda()
    fit = dict(epochs=3, batch_size=16, lr=5e-3)
    cv = T.cross_validate(emb, y, C, folds=3, seed=5, **fit)
    assert len(cv.folds) == 3 and sorted(np.concatenate([te for _, te in cv.folds]).tolist()) == list(range(N))
    for (tr_rows, te_rows), seed, head, acc in zip(cv.folds, cv.seeds, cv.heads, cv.accuracy):
        assert not set(tr_rows) & set(te_rows) and len(tr_rows) + len(te_rows) == N
        alone = T.fit_head(emb, y, C, rows=tr_rows, seed=seed, **fit)
        assert torch.equal(alone.weights, head.weights) and alone.loss == head.loss
        logits = emb.cpu().numpy()[te_rows].astype(np.float64) @ alone.kernel.astype(np.float64) + alone.bias.astype(np.float64)
        assert acc == float((logits.argmax(1) == y[te_rows]).mean())
    assert min(cv.accuracy) > 1.0 / C                        # separable clusters: better than chance on every held-out fold


# ---- train.py --freeze_backbone -----------------------------------------------------------------------------------------------------
def test_train_py_freeze_backbone(torch, tmp_path):
    from classifier.data import get_dataset
    from classifier.model import KWSModel
    from classifier.params import pr
    from kws_amd import transfer as T
    rng = np.random.default_rng(71)
    classes = ["background", "yes", "no"]
    proto = rng.standard_normal((3, pr.n_features, pr.feature_size, 1))
    for c, cls in enumerate(classes):
        d = tmp_path / "data" / "features" / cls
        d.mkdir(parents=True)
        for i in range(20):
            np.save(str(d / ("%02d.npy" % i)), (proto[c] + 0.5 * rng.standard_normal(proto[c].shape)).astype(np.float32))
    (tmp_path / "classes.txt").write_text("\n".join(classes) + "\n")
    ckpt = str(tmp_path / "twelve.npz")
    old = _kws_model("simple_gru", 12, 11)
    old.save_weights(ckpt)
    spec = importlib.util.spec_from_file_location("kws_train_main_freeze_gpu", os.path.join(os.path.dirname(os.path.dirname(__file__)),
                                                                                         "tf-keras-speech-commands_amd", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    logs = tmp_path / "logs"
    argv = ["--train_data_path", str(tmp_path / "data"), "--classes_path", str(tmp_path / "classes.txt"), "--model_type", "simple_gru",
            "--weights_path", ckpt, "--epochs", "2", "--batch_size", "16", "--val_split", "0.25", "--log_dir", str(logs)]
    for extra, msg in ((["--optimizer", "rmsprop"], "rmsprop"), (["--clipnorm", "1.0"], "clipnorm"), (["--average_type", "ema"], "average_type")):
        with pytest.raises(SystemExit, match=msg):
            train.main(argv + ["--freeze_backbone"] + extra)
    with pytest.raises(SystemExit, match="weights_path"):
        train.main([a for a in argv if a not in ("--weights_path", ckpt)] + ["--freeze_backbone"])
    np.random.seed(0)
    hist = train.main(argv + ["--freeze_backbone"])
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"])) and len(hist.history["val_accuracy"]) == 2
    # every backbone tensor of the saved model is the checkpoint's, bit for bit; the head has 3 classes
    z0, z1 = np.load(ckpt), np.load(str(logs / "trained_final.npz"))
    names = [n for n in z0["__order__"]]
    assert names == [n for n in z1["__order__"]]
    for n in names[:-2]:
        np.testing.assert_array_equal(z0[n], z1[n])
    assert z1["score_predict/kernel"].shape == (48, 3) and z1["score_predict/bias"].shape == (3,) and z0["score_predict/kernel"].shape == (48, 12)
    # the logged loss is fit_head's on the same split, embeddings and seeds
    np.random.seed(0)
    x_train, y_train, _, _ = get_dataset(str(tmp_path / "data"), classes, 0.25)
    m3 = KWSModel("simple_gru", 3)
    m3.load_weights(ckpt, by_name=True, skip_mismatch=True)
    emb = T.embed(m3, x_train)
    h = T.fit_head(emb, y_train, 3, epochs=1, batch_size=16, lr=1e-3, seed=0)
    h2 = T.fit_head(emb, y_train, 3, epochs=1, batch_size=16, lr=1e-3, seed=1, init=h, state=h.state)
    assert hist.history["loss"] == [h.loss[0], h2.loss[0]] and hist.history["accuracy"] == [h.accuracy[0], h2.accuracy[0]]
    np.testing.assert_array_equal(z1["score_predict/kernel"], h2.kernel)
