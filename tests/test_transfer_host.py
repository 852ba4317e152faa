"""Host-side checks of the transfer feature (include/kws.h: kws_model_embed_size, kws_head_fit_max_classes, kws_head_fit's argument
checks; kws_amd.transfer's validation) and of the reference and case table the GPU tests use (tests/transfer_ref.py,
tests/transfer_cases.py): no GPU."""
import ctypes

import numpy as np
import pytest

import transfer_cases as tc
import transfer_ref as tr
from kws_amd import lib as L
from oracle import model_oracle as mo


def _lib():
    return L.get_lib()


# ---- host-only entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layers,want", [("simple_cnn", None, 128), ("simple_cnn_lite", None, 128), ("simple_gru", None, 48),
                                              ("simple_lstm", None, 48), ("simple_gru", 2, 48)])
def test_embed_size(kind, layers, want):
    from kws_amd.model import ModelSpec
    spec = ModelSpec(kind, 7, 30, 20, layers)
    assert _lib().kws_model_embed_size(spec.handle) == want
    assert _lib().kws_model_embed_size(None) == 0


def test_max_classes():
    lim = {E: _lib().kws_head_fit_max_classes(E) for E in range(4, 129, 4)}
    assert lim[128] >= 64
    assert all(lim[E] >= 2 for E in lim)
    assert all(lim[a] >= lim[b] for a, b in zip(sorted(lim), sorted(lim)[1:])), lim         # wider embeddings never allow more classes
    for E, want in tc.MAX_CLASSES.items():
        assert lim[E] == want
    for E in (0, 2, 6, 130, 132, -4):
        assert _lib().kws_head_fit_max_classes(E) == 0


def _job(**kw):
    j = L.KwsHeadJob()
    j.order_offset, j.weight_offset, j.class_weight_offset, j.t0 = 0, 0, -1, 0
    j.n_order, j.batch, j.num_classes, j.ignore_index, j.optimizer = 32, 16, 12, 0, L.OPT_KINDS["adam"]
    j.lr, j.beta1, j.beta2, j.eps, j.momentum = 1e-3, 0.9, 0.999, 1e-7, 0.0
    for k, v in kw.items():
        setattr(j, k, v)
    return j


FAKE = 0x10000      # a non-null, aligned address: every case below must be refused before anything is read through it


def _call(jobs, E=128, J=None, N=200, **ptr):
    p = dict(emb=FAKE, labels=FAKE, order=FAKE, class_weights=None, jobs_dev=FAKE, weights=FAKE, slot_m=FAKE, slot_v=FAKE, stats=FAKE)
    p.update(ptr)
    arr = (L.KwsHeadJob * max(len(jobs), 1))(*jobs)
    return _lib().kws_head_fit(p["emb"], p["labels"], N, E, p["order"], p["class_weights"], arr if jobs is not None else None, p["jobs_dev"],
                               len(jobs) if J is None else J, p["weights"], p["slot_m"], p["slot_v"], p["stats"], None)


@pytest.mark.parametrize("what,kw,job", [
    ("J = 0", dict(J=0), {}), ("J < 0", dict(J=-3), {}),
    ("E = 0", dict(E=0), {}), ("E = 6", dict(E=6), {}), ("E = 132", dict(E=132), {}), ("E = -4", dict(E=-4), {}),
    ("batch = 0", {}, dict(batch=0)), ("batch < 0", {}, dict(batch=-1)),
    ("one class", {}, dict(num_classes=1)), ("no class", {}, dict(num_classes=0)),
    ("null emb", dict(emb=None), {}), ("null labels", dict(labels=None), {}), ("null order", dict(order=None), {}),
    ("null jobs_dev", dict(jobs_dev=None), {}), ("null weights", dict(weights=None), {}), ("null stats", dict(stats=None), {}),
    ("class weights named, array null", {}, dict(class_weight_offset=0)),
    ("negative n_order", {}, dict(n_order=-1)), ("momentum > 1", {}, dict(optimizer=0, momentum=1.5)), ("N = 0", dict(N=0), {}),
])
def test_head_fit_refuses_bad_arguments_without_a_device(what, kw, job):
    assert _call([_job(**job)], **kw) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


def test_head_fit_null_jobs():
    assert _lib().kws_head_fit(FAKE, FAKE, 200, 128, FAKE, None, None, FAKE, 1, FAKE, FAKE, FAKE, FAKE, None) == L.ERR_INVALID


@pytest.mark.parametrize("E", sorted(tc.MAX_CLASSES))
def test_head_fit_names_the_class_limit(E):
    lim = tc.MAX_CLASSES[E]
    assert _call([_job(num_classes=lim + 1)], E=E) == L.ERR_UNSUPPORTED
    assert str(lim) in _lib().kws_last_error().decode()
    assert _call([_job(), _job(num_classes=lim + 1)], E=E) == L.ERR_UNSUPPORTED         # any job of the launch


def test_head_fit_refuses_other_optimizers():
    assert _call([_job(optimizer=L.OPT_KINDS["rmsprop"])]) == L.ERR_UNSUPPORTED
    assert _call([_job(optimizer=7)]) == L.ERR_UNSUPPORTED


def test_job_struct_is_80_bytes():
    assert ctypes.sizeof(L.KwsHeadJob) == 80


# ---- kws_amd.transfer: ValueError before any device work ----------------------------------------------------------------------------
def test_python_validation():
    import torch
    from kws_amd import transfer as T
    emb = torch.zeros((20, 128), dtype=torch.float32)           # a CPU tensor: the device check comes last, so every other one is reachable
    y = np.arange(20) % 5
    with pytest.raises(ValueError, match="labels outside"):
        T.fit_head(emb, np.where(y == 4, 5, y), 5, epochs=1)
    with pytest.raises(ValueError, match="labels outside"):
        T.fit_head(emb, np.where(y == 4, -1, y), 5, epochs=1)
    with pytest.raises(ValueError, match="labels outside"):
        T.fit_head(emb, np.where(y == 4, 9, y), 5, epochs=1, ignore_index=3)
    with pytest.raises(ValueError, match="GPU"):
        T.fit_head(emb, np.where(y == 4, 9, y), 5, epochs=1, ignore_index=9)      # the ignored label may lie outside; then the device check
    for order in ([0, 20], [-1, 3]):
        with pytest.raises(ValueError, match="order entries outside"):
            T.fit_heads(emb, y, [dict(order=np.array(order), num_classes=5)])
    with pytest.raises(ValueError, match="order entries outside"):
        T.fit_head(emb, y, 5, epochs=1, rows=np.array([1, 2, 50]))
    for bad in (torch.zeros((20, 6)), torch.zeros((20, 132)), torch.zeros((20,)), torch.zeros((20, 128), dtype=torch.float64),
                torch.zeros((20, 256))[:, ::2], np.zeros((20, 128), np.float32), torch.zeros((0, 128))):
        with pytest.raises(ValueError, match="emb must|embedding width"):
            T.fit_head(bad, y, 5, epochs=1)
    with pytest.raises(ValueError, match="GPU"):
        T.fit_head(emb, y, 5, epochs=1)
    with pytest.raises(ValueError, match="2..64 classes"):
        T.fit_head(emb, y, 65, epochs=1)
    with pytest.raises(ValueError, match="classes"):
        T.fit_head(emb, y, 1, epochs=1)
    with pytest.raises(ValueError, match="adam.*sgd"):
        T.fit_head(emb, y, 5, epochs=1, optimizer="rmsprop")
    with pytest.raises(ValueError, match="labels for"):
        T.fit_head(emb, y[:-1], 5, epochs=1)
    with pytest.raises(ValueError, match="learning rates"):
        T.fit_head(emb, y, 5, epochs=3, lr=[1e-3, 1e-4])
    assert T.max_classes(128) == 64 and T.max_classes(6) == 0


def test_glorot_head():
    from kws_amd import transfer as T
    k, b = T.glorot_head(128, 12, seed=3)
    assert k.shape == (128, 12) and k.dtype == np.float32 and b.shape == (12,) and not b.any()
    assert np.abs(k).max() <= np.sqrt(6.0 / 140) and np.abs(k).max() > 0.9 * np.sqrt(6.0 / 140)
    np.testing.assert_array_equal(k, T.glorot_head(128, 12, seed=3)[0])


def test_epoch_orders_are_seeded_permutations():
    from kws_amd import transfer as T
    rows = np.array([3, 5, 8, 13, 21])
    a, b = T.epoch_orders(rows, 3, 7), T.epoch_orders(rows, 3, 7)
    rng = np.random.default_rng(7)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, rows[rng.permutation(5)])


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_reference_leaves_an_empty_job_alone():
    case = tc.CASE["empty"]
    d = tc.data(case)
    st = tr.HeadState(d["kernel"], d["bias"])
    st.m[0][:] = 0.25
    st.t = 5
    before = st.copy()
    assert tr.fit_launch(d["emb"], d["labels"], d["order"], case.batch, st) == (0.0, 0.0)
    for a, b in zip([st.kernel, st.bias] + st.m + st.v, [before.kernel, before.bias] + before.m + before.v):
        np.testing.assert_array_equal(a, b)
    assert st.t == 5


def test_reference_one_sample_by_hand():
    """E = 2, C = 2, one row, one Adam step and one SGD step written out"""
    x = np.array([[1.0, 2.0]])
    W, b = np.array([[0.1, -0.2], [0.3, 0.4]]), np.array([0.05, -0.05])
    z = x[0] @ W + b                                    # (0.75, 0.55)
    p = np.exp(z) / np.exp(z).sum()
    d = p - np.array([0.0, 1.0])                        # label 1
    gW, gb = np.outer(x[0], d), d
    st = tr.HeadState(W, b)
    loss, hits = tr.fit_launch(x, [1], [0], 4, st, optimizer="sgd", lr=0.5)
    assert abs(loss + np.log(p[1])) < 1e-15 and hits == 0.0         # class 0 has the larger logit
    np.testing.assert_allclose(st.kernel, W - 0.5 * gW, atol=1e-15, rtol=0)
    np.testing.assert_allclose(st.bias, b - 0.5 * gb, atol=1e-15, rtol=0)
    st = tr.HeadState(W, b)
    tr.fit_launch(x, [1], [0], 4, st, optimizer="adam", lr=1e-3)
    # first Adam step: m = 0.1 g, v = 0.001 g^2, lr_1 = lr sqrt(0.001) / 0.1: the move is lr g / (|g| + eps sqrt(1000)) ~ lr sign(g)
    lr1 = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    np.testing.assert_allclose(st.kernel, W - lr1 * 0.1 * gW / (np.sqrt(0.001 * gW * gW) + 1e-7), atol=1e-15, rtol=0)
    np.testing.assert_allclose(st.m[1], (1 - 0.9) * gb, atol=1e-17, rtol=0)
    assert st.t == 1
    # momentum: the second step moves by momentum * v + the new gradient step
    st = tr.HeadState(W, b)
    tr.fit_launch(x, [1, 1], [0, 0], 1, st, optimizer="sgd", lr=0.5, momentum=0.9)
    z2 = x[0] @ (W - 0.5 * gW) + (b - 0.5 * gb)
    d2 = np.exp(z2) / np.exp(z2).sum() - np.array([0.0, 1.0])
    np.testing.assert_allclose(st.bias, b - 0.5 * gb + (0.9 * (-0.5 * gb) - 0.5 * d2), atol=1e-15, rtol=0)


def test_reference_ignored_batch_still_decays_adam():
    case = tc.CASE["ignored-batch"]
    d = tc.data(case)
    st = tr.HeadState(d["kernel"], d["bias"])
    kw = tc.job_kw(case, d)
    tr.fit_launch(d["emb"], d["labels"], d["order"][:case.batch], case.batch, st, **kw)
    m1, w1 = st.m[0].copy(), st.kernel.copy()
    loss, _ = tr.fit_launch(d["emb"], d["labels"], d["order"][case.batch:2 * case.batch], case.batch, st, **kw)
    assert loss == 0.0
    np.testing.assert_allclose(st.m[0], 0.9 * m1, atol=1e-17, rtol=0)
    assert np.abs(st.kernel - w1).max() > 1e-5          # the weights move by the decayed momentum


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_seeds_are_insensitive_to_the_summation_order(case):
    """the check stated next to the seeds in tests/transfer_cases.py: a float32 run of the reference that sums every batch in the
    reversed row order stays within tol / 2 of ref64, and the loss sum's tol holds two float32 spacings of the sum"""
    d, ref64, tol = tc.expected(case)
    rev = tc.reference(case, d, np.float32, reverse=True)
    figures = {q: (float(np.abs(np.asarray(rev[q], np.float64) - ref64[q]).max()), tol[q]) for q in tc.QUANTITIES}
    print(case.name, figures)
    for q, (err, t) in figures.items():
        assert err <= 0.5 * t, (case.name, q, err, t)
    if case.n_order:
        assert tol["loss_sum"] >= 2 * np.spacing(np.float32(abs(float(ref64["loss_sum"]))))
