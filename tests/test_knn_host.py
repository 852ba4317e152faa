"""Host-side checks of the nearest-neighbour feature (include/kws.h: the argument checks of kws_rows_normalize, kws_knn_workspace_bytes,
kws_knn and kws_knn_vote; kws_amd.neighbors' validation) and of the reference and case table the GPU tests use (tests/knn_ref.py,
tests/knn_cases.py): no GPU."""
import numpy as np
import pytest

import knn_cases as kc
import knn_ref as kr
from kws_amd import lib as L

FAKE = 0x10000      # a non-null, aligned address: every case below must be refused before anything is read through it


def _lib():
    return L.get_lib()


# ---- the reference by hand ----------------------------------------------------------------------------------------------------
Q3 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])
R3 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])           # row 2 is a copy of row 0


def test_reference_dot_by_hand():
    idx, score = kr.knn(Q3, R3, 2, kr.DOT)
    # query 0: rows 0 and 2 score 1 (the lower index first), row 1 scores 0
    # query 1: row 1 scores 2, rows 0 and 2 score 0: row 0 before row 2
    # query 2: all three score 1: rows 0, 1
    np.testing.assert_array_equal(idx, [[0, 2], [1, 0], [0, 1]])
    np.testing.assert_array_equal(score, [[1.0, 1.0], [2.0, 0.0], [1.0, 1.0]])


def test_reference_l2_by_hand():
    idx, score = kr.knn(Q3, R3, 3, kr.L2)
    # query 0: distances 0, 2, 0 -> rows 0, 2, 1;  query 1: 5, 1, 5 -> 1, 0, 2;  query 2: 1, 1, 1 -> 0, 1, 2
    np.testing.assert_array_equal(idx, [[0, 2, 1], [1, 0, 2], [0, 1, 2]])
    np.testing.assert_array_equal(score, [[0.0, 0.0, 2.0], [1.0, 5.0, 5.0], [1.0, 1.0, 1.0]])


def test_reference_exclusion_and_tail():
    idx, score = kr.knn(Q3, R3, 3, kr.DOT, exclude=np.array([0, -1, 2]))
    np.testing.assert_array_equal(idx, [[2, 1, -1], [1, 0, 2], [0, 1, -1]])
    assert score[0, 2] == -np.inf and score[2, 2] == -np.inf and score[1, 2] == 0.0
    idx, score = kr.knn(Q3, R3, 4, kr.L2)
    assert (idx[:, 3] == -1).all() and (score[:, 3] == np.inf).all()


def test_reference_vote_by_hand():
    labels = np.array([2, 0, 0, 1])
    idx = np.array([[0, 1, 2], [0, 3, -1], [-1, -1, -1], [0, 3, 1]])
    score = np.array([[0.9, 0.3, 0.3], [0.5, 0.5, -np.inf], [-np.inf] * 3, [-1.0, 0.25, 0.25]])
    pred, support, own = kr.vote(idx, score, labels, 3, own_labels=np.array([2, 2, 0, 1]))
    # row 0: class 0 has two votes of three; row 1: classes 2 and 1 tie at one vote, the lower class wins; row 2: no vote;
    # row 3: three classes with one vote each: class 0
    np.testing.assert_array_equal(pred, [0, 1, -1, 0])
    np.testing.assert_allclose(support, [2 / 3, 0.5, 0.0, 1 / 3])
    np.testing.assert_allclose(own, [1 / 3, 0.5, 0.0, 1 / 3])
    pred, support = kr.vote(idx, score, labels, 3, weighted=True)
    # row 0: class 2 weighs 0.9 against 0.6; row 3: the negative score counts 0, classes 1 and 0 tie at 0.25: class 0
    np.testing.assert_array_equal(pred, [2, 1, -1, 0])
    np.testing.assert_allclose(support, [0.6, 0.5, 0.0, 0.5])


def test_reference_normalize_duplicates_and_issues():
    emb = np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [6.0, 8.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 2.0, 0.1]])
    unit, norms = kr.normalize(emb)
    np.testing.assert_allclose(norms, [5.0, 0.0, 10.0, 1.0, np.sqrt(4.01)])
    np.testing.assert_array_equal(unit[1], 0.0)
    np.testing.assert_allclose(unit[0], [0.6, 0.8, 0.0, 0.0])
    a, b, c = kr.duplicates(emb, threshold=0.9995, k=2)
    assert a.tolist() == [0] and b.tolist() == [2] and abs(c[0] - 1.0) < 1e-12             # once, row_a < row_b; 3 / 4 have cosine 0.9988
    a, b, c = kr.duplicates(emb, emb[2:3], threshold=0.9995, k=1)
    assert a.tolist() == [0, 2] and b.tolist() == [0, 0]
    rows, label, sug, own, sup = kr.label_issues(emb, [0, 0, 1, 1, 1], 2, k=1)
    # row 0's nearest is row 2 (label 1), row 2's nearest is row 0 (label 0); the zero row 1 scores 0 against everyone: its nearest is the
    # lowest other index, row 0, of its own label
    assert rows.tolist() == [0, 2] and sug.tolist() == [1, 0] and own.tolist() == [0.0, 0.0] and sup.tolist() == [1.0, 1.0]


def test_case_table():
    names = [(s.Q, s.N) for s in kc.SHAPES]
    assert names == [(1, 1), (1, 5), (33, 31), (129, 257), (130, 1025)]
    assert kc.WIDTHS == (4, 48, 128) and kc.KS == (1, 5, 32, 64) and set(kc.SLICES) == {0, 1, 2, 7, 64}
    assert all(s.why for s in kc.SHAPES + kc.EDGE_SHAPES)
    q, r, ex = kc.data(130, 1025, 48)
    assert np.abs(q).max() <= 4 and np.abs(r).max() <= 4 and (q == np.round(q)).all()
    assert (r[1] == r[1024]).all() and (r[1023] == r[0]).all() and (ex == -1).sum() == 1
    idx, score = kc.expected(130, 1025, 48, kr.L2, False)
    assert idx[0, :2].tolist() == [0, 1023] and score[0, 1] == 0  # query 0 is row 0: the copy ties with it, the lower index first
    ties = sum(len(set(score[i])) < 64 for i in range(130))
    assert ties > 100                                               # equal scores in nearly every row


# ---- the C ABI refuses bad arguments before any device work -----------------------------------------------------------------------
def _knn(Q=10, N=100, E=128, metric=0, k=5, slices=1, ws_bytes=0, **ptr):
    p = dict(queries=FAKE, refs=FAKE, exclude=None, idx=FAKE, score=FAKE, ws=None)
    p.update(ptr)
    return _lib().kws_knn(p["queries"], Q, p["refs"], N, E, metric, k, p["exclude"], slices, p["idx"], p["score"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("what,kw", [
    ("E = 0", dict(E=0)), ("E = 2", dict(E=2)), ("E = 6", dict(E=6)), ("E = 132", dict(E=132)), ("k = 0", dict(k=0)), ("k = 65", dict(k=65)),
    ("metric 2", dict(metric=2)), ("metric -1", dict(metric=-1)), ("slices -1", dict(slices=-1)), ("slices 1025", dict(slices=1025)),
    ("N = 0", dict(N=0)), ("N = 2^31", dict(N=2 ** 31)), ("Q < 0", dict(Q=-1)),
    ("null queries", dict(queries=None)), ("null refs", dict(refs=None)), ("null idx", dict(idx=None)), ("null score", dict(score=None)),
    ("misaligned refs", dict(refs=FAKE + 4)), ("misaligned queries", dict(queries=FAKE + 8)),
])
def test_knn_refuses_bad_arguments_without_a_device(what, kw):
    assert _knn(**kw) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


def test_knn_workspace():
    lib = _lib()
    assert lib.kws_knn_workspace_bytes(10, 100, 128, 5, 1) == 0
    need = lib.kws_knn_workspace_bytes(10, 100, 128, 5, 7)
    assert 7 * 10 * 5 * 8 <= need < 7 * 10 * 5 * 8 + 256          # slices x Q x k pairs plus alignment
    assert _knn(slices=7) == L.ERR_WORKSPACE                        # none given
    assert _knn(slices=7, ws=FAKE, ws_bytes=need - 1) == L.ERR_WORKSPACE
    assert b"workspace" in lib.kws_last_error()
    # the library's own choice: one query against many rows is cut up, a large self-search is not
    assert lib.kws_knn_workspace_bytes(1, 65536, 128, 10, 0) > 0
    assert lib.kws_knn_workspace_bytes(65536, 65536, 128, 10, 0) == 0
    assert _knn(Q=1, N=65536, slices=0) == L.ERR_WORKSPACE
    for kw in (dict(E=6), dict(E=0), dict(E=2), dict(E=132), dict(k=0), dict(k=65), dict(slices=-1), dict(N=0), dict(Q=-1)):
        a = dict(Q=10, N=100, E=128, k=5, slices=1)
        a.update(kw)
        assert lib.kws_knn_workspace_bytes(a["Q"], a["N"], a["E"], a["k"], a["slices"]) == L.ERR_INVALID, kw


def test_q_zero_is_ok():
    assert _knn(Q=0) == 0
    assert _lib().kws_knn_vote(FAKE, FAKE, 0, 5, FAKE, 100, 5, 0, None, FAKE, FAKE, None, None) == 0
    assert _lib().kws_rows_normalize(FAKE, 0, 128, FAKE, None, None) == 0
    assert _lib().kws_knn_workspace_bytes(0, 100, 128, 5, 7) == 0


def _vote(Q=10, k=5, N=100, C=5, weighted=0, **ptr):
    p = dict(idx=FAKE, score=FAKE, labels=FAKE, own_labels=None, pred=FAKE, support=FAKE, own=None)
    p.update(ptr)
    return _lib().kws_knn_vote(p["idx"], p["score"], Q, k, p["labels"], N, C, weighted, p["own_labels"], p["pred"], p["support"], p["own"], None)


@pytest.mark.parametrize("what,kw", [
    ("C = 1", dict(C=1)), ("C = 1025", dict(C=1025)), ("C = 0", dict(C=0)), ("k = 0", dict(k=0)), ("k = 65", dict(k=65)), ("N = 0", dict(N=0)),
    ("Q < 0", dict(Q=-2)), ("null idx", dict(idx=None)), ("null labels", dict(labels=None)), ("null pred", dict(pred=None)),
    ("null support", dict(support=None)), ("weighted without scores", dict(weighted=1, score=None)),
    ("own without own_labels", dict(own=FAKE)), ("own_labels without own", dict(own_labels=FAKE)),
])
def test_vote_refuses_bad_arguments_without_a_device(what, kw):
    assert _vote(**kw) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


@pytest.mark.parametrize("what,args", [
    ("E = 0", (FAKE, 10, 0, FAKE, None)), ("E = 2", (FAKE, 10, 2, FAKE, None)), ("E = 6", (FAKE, 10, 6, FAKE, None)),
    ("E = 132", (FAKE, 10, 132, FAKE, None)), ("N < 0", (FAKE, -1, 128, FAKE, None)), ("null x", (None, 10, 128, FAKE, None)),
    ("null out", (FAKE, 10, 128, None, None)), ("misaligned", (FAKE + 4, 10, 128, FAKE, None)),
])
def test_normalize_refuses_bad_arguments_without_a_device(what, args):
    assert _lib().kws_rows_normalize(*args, None) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


# ---- kws_amd.neighbors: ValueError before any device work ---------------------------------------------------------------------------
def test_python_validation():
    import torch
    from kws_amd import neighbors as nb
    emb = torch.zeros((20, 128), dtype=torch.float32)               # host tensors: the device check comes last, every other one is reachable
    y = np.arange(20) % 5
    bad_embs = (torch.zeros((20, 6)), torch.zeros((20, 132)), torch.zeros((20, 2)), torch.zeros((20, 0)), torch.zeros((20,)),
                torch.zeros((20, 128), dtype=torch.float64), torch.zeros((20, 256))[:, ::2], np.zeros((20, 128), np.float32))
    for bad in bad_embs:
        with pytest.raises(ValueError, match="must be a contiguous|embedding width"):
            nb.knn(bad, emb, 3)
        with pytest.raises(ValueError, match="must be a contiguous|embedding width"):
            nb.knn(emb, bad, 3)
        with pytest.raises(ValueError, match="must be a contiguous|embedding width"):
            nb.normalize(bad)
        with pytest.raises(ValueError, match="must be a contiguous|embedding width"):
            nb.label_issues(bad, y, 5)
        with pytest.raises(ValueError, match="must be a contiguous|embedding width"):
            nb.duplicates(bad)
    with pytest.raises(ValueError, match="must be a contiguous"):
        nb.knn(emb, torch.zeros((0, 128)), 3)                       # no reference rows
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="neighbours"):
            nb.knn(emb, emb, k)
        with pytest.raises(ValueError, match="neighbours"):
            nb.label_issues(emb, y, 5, k=k)
    with pytest.raises(ValueError, match="metric"):
        nb.knn(emb, emb, 3, metric="manhattan")
    for s in (-1, 1025):
        with pytest.raises(ValueError, match="slices"):
            nb.knn(emb, emb, 3, slices=s)
    with pytest.raises(ValueError, match="wide"):
        nb.knn(torch.zeros((20, 48)), emb, 3)
    with pytest.raises(ValueError, match="exclude_self"):
        nb.knn(torch.zeros((19, 128)), emb, 3, exclude_self=True)
    for C in (1, 1025):
        with pytest.raises(ValueError, match="classes"):
            nb.knn_predict(emb, y, emb, 3, C)
        with pytest.raises(ValueError, match="classes"):
            nb.label_issues(emb, y, C)
    with pytest.raises(ValueError, match="outside"):
        nb.label_issues(emb, np.where(y == 4, 5, y), 5)
    with pytest.raises(ValueError, match="outside"):
        nb.knn_predict(emb, np.where(y == 4, -1, y), emb, 3, 5)
    with pytest.raises(ValueError, match="labels for"):
        nb.label_issues(emb, y[:-1], 5)
    with pytest.raises(ValueError, match="integers"):
        nb.label_issues(emb, y.astype(np.float32), 5)
    with pytest.raises(ValueError, match="no cosine"):
        nb.duplicates(emb, threshold=1.5)
    idx, score = torch.zeros((20, 3), dtype=torch.int32), torch.zeros((20, 3))
    with pytest.raises(ValueError, match="not with metric 'l2'"):
        nb.vote(idx, score, y, 5, weighted=True, metric="l2")
    with pytest.raises(ValueError, match="idx must be"):
        nb.vote(idx.long(), score, y, 5)
    with pytest.raises(ValueError, match="idx is"):
        nb.vote(idx, score[:, :2].contiguous(), y, 5)
    # and last of all, the host tensors themselves
    for call in (lambda: nb.knn(emb, emb, 3), lambda: nb.normalize(emb), lambda: nb.label_issues(emb, y, 5), lambda: nb.duplicates(emb),
                 lambda: nb.duplicates(emb, emb), lambda: nb.knn_predict(emb, y, emb, 3, 5), lambda: nb.vote(idx, score, y, 5)):
        with pytest.raises(ValueError, match="GPU"):
            call()
