"""kws_heads_apply on the GPU (include/kws.h, the head-bank block; csrc/kws_heads.hip) and what is wired to it: kws_amd.transfer.HeadBank
/ score_heads and the `heads=` arguments of kws_amd.stream.StreamServer / StreamBatch / scan.

Logits are held to the rigorous bound of the float32 chain against the float64 reference (tests/head_bank_ref.py), probabilities to
2^-16 against the float64 softmax of the RETURNED logits (tests/head_bank_cases.py derives it), pred to the arg-max of the returned
logits exactly.  Wherever two device paths must agree -- a pair alone and among others, the run route and the per-row route, a slot
among slots of other heads and in a server of its own -- the comparison is bit for bit."""
import numpy as np
import pytest

import geometry_cases as gc
import head_bank_cases as hc
import head_bank_ref as ref

pytestmark = pytest.mark.gpu
T = hc.T


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def bank_of(heads, max_classes=None, capacity=None):
    from kws_amd.transfer import HeadBank
    bank = HeadBank(heads[0][0].shape[0], capacity or len(heads), max_classes or max(h[1].shape[0] for h in heads if h is not None))
    for i, h in enumerate(heads):
        if h is not None:
            bank.set(i, h)
    return bank


def run(torch, bank, emb, ids, rows=None, want=("logits", "probs", "pred")):
    """-> the outputs as numpy arrays; emb may be a numpy array or a device tensor"""
    e = emb if isinstance(emb, torch.Tensor) else torch.from_numpy(emb).cuda()
    return [v.cpu().numpy() for v in bank.apply(e, ids, rows=rows, want=want)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(got, want, msg=""):
    for g, w, name in zip(got, want, ("logits", "probs", "pred")):
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s %s" % (name, msg))


def check_against_reference(emb, heads, ids, Cmax, got, rows=None, msg=""):
    """logits within the chain's bound of the float64 reference, probabilities within 2^-16 of the float64 softmax of the returned
    logits, pred their arg-max (tie: lower class), padded columns exactly zero -> (max logit error / bound, max probability error)"""
    lg, pr, pd = got
    w_lg, w_bd, _, w_pd = ref.apply(emb, heads, ids, Cmax, rows)
    err = np.abs(lg.astype(np.float64) - w_lg)
    assert (err <= w_bd).all(), "%s: logit error %.3g over its bound %.3g" % (msg, err.max(), w_bd[err > w_bd].min())
    worst = float((err / np.maximum(w_bd, 1e-300)).max())
    e_pr = 0.0
    for r in range(lg.shape[0]):
        if w_pd[r] < 0:
            assert pd[r] == -1 and not lg[r].any() and not pr[r].any(), (msg, r)
            continue
        C = heads[int(ids[r])][1].shape[0]
        assert not lg[r, C:].any() and not pr[r, C:].any(), (msg, r)          # the padded columns: exactly zero
        want = ref.softmax(lg[r, :C])
        e_pr = max(e_pr, float(np.abs(pr[r, :C] - want).max()))
        assert pd[r] == ref.argmax_low(lg[r, :C]), (msg, r)
    assert e_pr <= hc.PROB_ATOL, "%s: probability error %.3g" % (msg, e_pr)
    return worst, e_pr


@pytest.mark.parametrize("case", hc.logit_cases(), ids=hc.case_id)
def test_logits_probabilities_and_pred_against_the_reference(torch, case):
    E, classes = case
    H, Cmax = len(classes), max(classes)
    emb, heads = hc.make_case(E, classes, max(hc.ROW_COUNTS), seed=100 + E + sum(classes))
    bank = bank_of(heads)
    emb_d = torch.from_numpy(emb).cuda()
    worst = (0.0, 0.0)
    for R in hc.ROW_COUNTS:
        for ids in (hc.cyclic_ids(R, H), hc.block_ids(R, H)):                  # a head per row; tiles of one head (the run route)
            got = run(torch, bank, emb_d, ids)
            w = check_against_reference(emb, heads, ids, Cmax, got, msg="R = %d" % R)
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print("FIGURES | %s | logit error at most %.3g of its bound, probability error at most %.3g" % ((hc.case_id(case),) + worst))


INDEPENDENCE = [(128, (3, 5, 12, 12, 7, 31, 2, 9)), (48, (2, 128, 12, 64, 5, 3, 100, 8)), (4, (256, 3, 129, 2, 65, 7, 64, 200))]


@pytest.mark.parametrize("case", INDEPENDENCE, ids=hc.case_id)
def test_a_rows_bits_depend_on_its_embedding_and_its_head_alone(torch, case):
    E, classes = case
    H, Cmax = len(classes), max(classes)
    rows, ids = hc.independence_pairs(H)
    P = rows.size
    emb, heads = hc.make_case(E, classes, P, seed=7 + E)
    bank = bank_of(heads)
    emb_d = torch.from_numpy(emb).cuda()
    want = run(torch, bank, emb_d, ids)                                       # sorted by head: the runs straddle and fill tiles
    check_against_reference(emb, heads, ids, Cmax, want, msg="sorted")
    same_bits(run(torch, bank, emb_d, ids), want, "the same launch twice")
    # alone
    alone = [run(torch, bank, emb_d, ids[i:i + 1], rows=rows[i:i + 1]) for i in range(P)]
    same_bits([np.concatenate([a[k] for a in alone]) for k in range(3)], want, "alone")
    # every row of a batch a different head
    for b in hc.distinct_batches(ids):
        got = run(torch, bank, emb_d, ids[b], rows=rows[b])
        same_bits(got, [w[b] for w in want], "distinct heads")
    # descending head order
    got = run(torch, bank, emb_d, ids[::-1].copy(), rows=rows[::-1].copy())
    same_bits(got, [w[::-1] for w in want], "descending")
    # through `rows` into a permuted embedding matrix, and key -> head_of_key with key_stride = 8
    rng = np.random.default_rng(E)
    perm = rng.permutation(P + 3)[:P]                                          # pair i's embedding lies in row perm[i] of a larger matrix
    big = np.zeros((P + 3, E), np.float32)
    big[perm] = emb
    K = 3 * H
    head_of_key = rng.integers(0, H, K).astype(np.int32)
    head_of_key[:H] = rng.permutation(H)                                       # every head has a key
    key = np.array([rng.choice(np.flatnonzero(head_of_key == h)) for h in ids], np.int32)
    table = rng.integers(-5, 5, (P, 8)).astype(np.int32)
    table[:, 0] = key
    out = bank.launch(torch.from_numpy(big).cuda(), P, torch.from_numpy(table).cuda(), key_stride=8,
                      head_of_key=torch.from_numpy(head_of_key).cuda(), rows=torch.from_numpy(perm.astype(np.int32)).cuda(),
                      want=("logits", "probs", "pred"))
    same_bits([v.cpu().numpy() for v in out], want, "rows / key / head_of_key")


def test_exact_ties_go_to_the_lower_class(torch):
    rng = np.random.default_rng(3)
    E, N = 48, 2 * T + 3
    emb = rng.standard_normal((N, E)).astype(np.float32)
    heads = []
    for C, (a, b) in ((12, (4, 9)), (128, (5, 69)), (128, (70, 3)), (3, (0, 2))):      # neighbours in a wave, c and c + 64 of one lane, ..
        k = (0.05 * rng.standard_normal((E, C))).astype(np.float32)
        bias = np.zeros(C, np.float32)
        k[:, b] = k[:, a]
        bias[a] = bias[b] = 3.0                                                 # the two equal columns are the largest by far
        heads.append((k, bias))
    bank = bank_of(heads)
    for ids in (hc.cyclic_ids(N, 4), hc.block_ids(N, 4)):
        lg, pr, pd = run(torch, bank, emb, ids)
        for r in range(N):
            a, b = ((4, 9), (5, 69), (3, 70), (0, 2))[int(ids[r])]
            assert lg[r, a] == lg[r, b] == lg[r].max() and pd[r] == a, (r, ids[r])
            assert pr[r, a] == pr[r, b]


def test_padded_columns_are_zero_and_cannot_win(torch):
    rng = np.random.default_rng(4)
    E, N, Cmax = 128, T + 2, 8
    emb = np.abs(rng.standard_normal((N, E))).astype(np.float32)
    k = (-0.01 * np.abs(rng.standard_normal((E, 3)))).astype(np.float32)
    heads = [(k, np.array([-5.0, -4.0, -6.0], np.float32))]                     # every logit is negative: a padded 0 would be the maximum
    bank = bank_of(heads, max_classes=Cmax)
    for ids in (np.zeros(N, np.int32), np.zeros(1, np.int32)):
        got = run(torch, bank, emb, ids)
        lg, pr, pd = got
        assert (lg[:, :3] < 0).all() and not lg[:, 3:].any() and not pr[:, 3:].any()
        assert (pd == np.argmax(lg[:, :3], axis=1)).all() and (np.argmax(pr, axis=1) == pd).all()
        assert np.abs(pr.sum(axis=1) - 1).max() < 1e-5
        check_against_reference(emb, heads, ids, Cmax, got, msg="negative logits")


def test_clamping_gives_zero_rows_and_leaves_the_neighbours(torch):
    E, classes = 48, (3, 5, 12)
    R = 2 * T + 5
    emb, heads = hc.make_case(E, classes, R, seed=21)
    bank = bank_of(heads + [heads[1], heads[0]], capacity=5)
    bank.remove(3)                                                             # slot 3 was filled and is empty again; slot 4's offset moves below
    emb_d = torch.from_numpy(emb).cuda()
    ids = hc.cyclic_ids(R, 3)
    clean = run(torch, bank, emb_d, ids)
    check_against_reference(emb, heads, ids, 12, clean)

    def expect(got, bad, msg):
        for k, name in enumerate(("logits", "probs", "pred")):
            keep = np.setdiff1d(np.arange(R), bad)
            np.testing.assert_array_equal(bits(got[k][keep]), bits(clean[k][keep]), err_msg="%s: neighbours' %s" % (msg, name))
        assert not got[0][bad].any() and not got[1][bad].any() and (got[2][bad] == -1).all(), msg

    bad = np.array([0, 5, T - 1, T, R - 1])
    for what, value in (("head id -1", -1), ("head id H", 5), ("an empty slot", 3), ("a head id far outside", 2 ** 30)):
        x = ids.copy()
        x[bad] = value
        expect(run(torch, bank, emb_d, x), bad, what)
    rows = np.arange(R, dtype=np.int32)
    for what, value in (("row N", R), ("row -1", -1), ("a row far outside", 2 ** 30)):
        x = rows.copy()
        x[bad] = value
        expect(run(torch, bank, emb_d, ids, rows=x), bad, what)
    # keys outside [0, K)
    K = 7
    head_of_key = np.array([0, 1, 2, 0, 1, 2, 0], np.int32)
    key = (ids + 3 * (np.arange(R) % 2)).astype(np.int32)
    for what, value in (("key K", K), ("key -1", -1)):
        x = key.copy()
        x[bad] = value
        got = bank.launch(emb_d, R, torch.from_numpy(x).cuda(), head_of_key=torch.from_numpy(head_of_key).cuda(),
                          want=("logits", "probs", "pred"))
        expect([v.cpu().numpy() for v in got], bad, what)
    # an offset whose head would run past weights_count, and a negative one: slot 4 holds head 0's weights
    x = ids.copy()
    x[bad] = 4
    moved = run(torch, bank, emb_d, x)
    same = [c.copy() for c in clean]
    for k in range(3):
        same[k][bad] = run(torch, bank, emb_d, np.zeros(R, np.int32))[k][bad]
    same_bits(moved, same, "slot 4 is head 0")
    for off in (bank.count - (E + 1) * 3 + 1, bank.count, -4):
        bank.head_offset[4] = off
        expect(run(torch, bank, emb_d, x), bad, "offset %d" % off)
    bank.head_offset[4] = bank.count - (E + 1) * 3                              # the last place it fits: the zeros at the array's end
    got = run(torch, bank, emb_d, x)
    assert (got[2][bad] == 0).all() and np.abs(got[1][bad][:, :3] - 1.0 / 3).max() < 1e-6 and not got[1][bad][:, 3:].any() and not got[0][bad].any()
    # a class count outside 2 .. Cmax
    for c in (1, 13, -3):
        bank.head_classes[1] = c
        expect(run(torch, bank, emb_d, ids), np.flatnonzero(ids == 1), "classes %d" % c)


# ---- the streaming stack -----------------------------------------------------------------------------------------------------------
NAMES = {3: ["background", "up", "down"], 5: ["background", "a", "b", "c", "d"], 12: ["background"] + ["w%d" % i for i in range(11)]}
HEAD_CLASSES = (3, 5, 12)
SLOT_HEADS = (2, 0, 1, 0, 2, 1)
_MODELS = {}


def model_of(kind):
    """(pr, device model) on a tiny geometry: simple_cnn on 14 frames x 20 coefficients, simple_gru on 9 x 20"""
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    if kind not in _MODELS:
        g = gc.ROW["tuned-14" if kind == "simple_cnn" else "gen1-9"]
        assert gc.cnn_accepts(g) == (kind == "simple_cnn")
        spec = ModelSpec(kind, 5, g.frames, g.n_mfcc)
        dm = DeviceModel(spec)
        dm.set_weights(init_weights(spec, seed=3))
        _MODELS[kind] = (gc.params(g), dm)
    return _MODELS[kind]


def stream_heads(E, seed=0):
    """three heads of 3, 5 and 12 classes whose logits on unit-scale embeddings stay moderate"""
    rng = np.random.default_rng(seed)
    return [((rng.uniform(-1, 1, (E, C)) / np.sqrt(E)).astype(np.float32), rng.uniform(-0.5, 0.5, C).astype(np.float32)) for C in HEAD_CLASSES]


def named_bank(heads):
    from kws_amd.transfer import HeadBank
    return HeadBank.from_fits(heads, names=[NAMES[h[1].shape[0]] for h in heads])


def pcm_of(rng, n, level=3000.0):
    return np.clip(rng.normal(0, level, n), -32768, 32767).astype(np.int16)


def ragged_schedule(S, pushes, chunk, seed):
    """per push (slots, chunks): slots absent, lengths differing, order shuffled"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(pushes):
        slots = [s for s in range(S) if rng.random() < 0.7] or [int(rng.integers(S))]
        rng.shuffle(slots)
        out.append((slots, [pcm_of(rng, int(rng.integers(1, chunk + 1)), float(rng.choice([300.0, 3000.0, 9000.0]))) for _ in slots]))
    out.append((list(range(S)), [pcm_of(rng, chunk) for _ in range(S)]))       # and one push that names every slot
    return out


@pytest.mark.parametrize("kind", ["simple_cnn", "simple_gru"])
def test_server_applies_each_slots_head_to_the_backbones_embedding(torch, kind):
    from kws_amd.stream import StreamServer
    pr, dm = model_of(kind)
    E, S, chunk = dm.embed_size, len(SLOT_HEADS), 800
    heads = stream_heads(E)
    bank = named_bank(heads)
    srv = StreamServer(pr, dm, S, chunk_size=chunk, heads=bank)
    assert [srv.open(head=h) for h in SLOT_HEADS] == list(range(S))
    assert srv.slot_head.cpu().tolist() == list(SLOT_HEADS) and srv.head_class_names(SLOT_HEADS[0]) == NAMES[12]
    e_max, launches, live = 0.0, 0, False
    for slots, chunks in ragged_schedule(S, 10, chunk, seed=1):
        index, score, fired = srv.push(slots, chunks)
        A = len(slots)
        assert srv.launches - launches in (5, 6)                               # the head stage is counted
        launches = srv.launches
        emb = dm.embed(srv._feat[:A]).cpu().numpy()
        ids = np.array([SLOT_HEADS[s] for s in slots])
        w_lg, w_bd, w_pr, w_pd = ref.apply(emb, heads, ids, 12)
        probs = srv.probs.cpu().numpy()
        assert probs.shape == (A, 12)
        # a logit error d moves a probability by at most (e^{2 d} - 1) p <= 2.1 d; on top the softmax's own 2^-16
        tol = 2.1 * float(w_bd.max()) + hc.PROB_ATOL
        err = float(np.abs(probs - w_pr).max())
        e_max = max(e_max, err)
        assert err <= tol, (err, tol)
        for a in range(A):
            assert not probs[a, HEAD_CLASSES[ids[a]]:].any()
        top = np.argmax(probs, axis=1)
        np.testing.assert_array_equal(index.cpu().numpy(), top)
        live = live or bool(emb.any())
    assert live and emb.any()                                                  # rows did arrive: the heads saw more than zeros
    print("FIGURES | server %s | probabilities within %.3g of the reference heads on the device's embeddings" % (kind, e_max))


def test_server_is_bit_identical_to_one_server_per_head(torch):
    from kws_amd.stream import StreamServer
    from kws_amd.transfer import HeadBank
    pr, dm = model_of("simple_cnn")
    S, chunk = len(SLOT_HEADS), 800
    heads = stream_heads(dm.embed_size, seed=5)
    srv = StreamServer(pr, dm, S, chunk_size=chunk, heads=named_bank(heads), sensitivity=0.4, trigger_level=2)
    assert [srv.open(head=h) for h in SLOT_HEADS] == list(range(S))
    single, local = [], {}
    for h in range(3):
        mine = [s for s in range(S) if SLOT_HEADS[s] == h]
        one = StreamServer(pr, dm, len(mine), chunk_size=chunk, heads=HeadBank.from_fits([heads[h]]), sensitivity=0.4, trigger_level=2)
        for s in mine:
            local[s] = one.open()
        single.append(one)
    for slots, chunks in ragged_schedule(S, 14, chunk, seed=2):
        got = [v.cpu().numpy().copy() for v in srv.push(slots, chunks)]
        probs = srv.probs.cpu().numpy()
        for h in range(3):
            at = [a for a, s in enumerate(slots) if SLOT_HEADS[s] == h]
            if not at:
                continue
            want = [v.cpu().numpy() for v in single[h].push([local[slots[a]] for a in at], [chunks[a] for a in at])]
            C = HEAD_CLASSES[h]
            np.testing.assert_array_equal(bits(probs[at][:, :C]), bits(single[h].probs.cpu().numpy()))
            assert not probs[at][:, C:].any()
            np.testing.assert_array_equal(got[0][at], want[0])
            np.testing.assert_array_equal(bits(got[1][at]), bits(want[1]))
            np.testing.assert_array_equal(got[2][at], want[2])
    for h in range(3):
        mine = [s for s in range(S) if SLOT_HEADS[s] == h]
        np.testing.assert_array_equal(srv.state[mine].cpu().numpy(), single[h].state.cpu().numpy())


def test_a_head_is_swapped_between_two_pushes(torch):
    from kws_amd.stream import StreamServer
    pr, dm = model_of("simple_gru")
    S, chunk = len(SLOT_HEADS), 800
    heads = stream_heads(dm.embed_size, seed=6)
    a, b = (StreamServer(pr, dm, S, chunk_size=chunk, heads=named_bank(heads)) for _ in range(2))
    for srv in (a, b):
        assert [srv.open(head=h) for h in SLOT_HEADS] == list(range(S))
    sched = ragged_schedule(S, 6, chunk, seed=3)
    for slots, chunks in sched[:-1]:
        a.push(slots, chunks)
        b.push(slots, chunks)
        np.testing.assert_array_equal(bits(a.probs.cpu().numpy()), bits(b.probs.cpu().numpy()))
    new = stream_heads(dm.embed_size, seed=60)[1]
    a.heads.set(1, new, NAMES[5])                                              # no stop, no synchronisation: the next push sees it
    slots, chunks = sched[-1]                                                  # names every slot
    a.push(slots, chunks)
    b.push(slots, chunks)
    pa, pb = a.probs.cpu().numpy(), b.probs.cpu().numpy()
    swapped = [i for i, s in enumerate(slots) if SLOT_HEADS[s] == 1]
    others = [i for i, s in enumerate(slots) if SLOT_HEADS[s] != 1]
    np.testing.assert_array_equal(bits(pa[others]), bits(pb[others]))
    assert all((pa[i] != pb[i]).any() for i in swapped) and len(swapped) == 2
    emb = a.model.embed(a._feat[:S]).cpu().numpy()
    want = ref.apply(emb[swapped], [new], [0] * len(swapped), 12)[2]
    assert np.abs(pa[swapped] - want).max() <= 1e-5


def test_stream_batch_takes_a_head_per_stream(torch):
    from kws_amd.stream import StreamBatch, StreamServer
    pr, dm = model_of("simple_cnn")
    S, chunk = len(SLOT_HEADS), 512
    bank = named_bank(stream_heads(dm.embed_size, seed=8))
    sb = StreamBatch(pr, dm, S, chunk_size=chunk, heads=bank, stream_heads=list(SLOT_HEADS))
    srv = StreamServer(pr, dm, S, chunk_size=chunk, heads=bank)
    slots = [srv.open(head=h) for h in SLOT_HEADS]
    rng = np.random.default_rng(8)
    for t in range(8):
        pcm = np.stack([pcm_of(rng, chunk) for _ in range(S)])
        want = [v.cpu().numpy().copy() for v in srv.push(slots, pcm)]
        got = [v.cpu().numpy() for v in sb.push(pcm)]
        np.testing.assert_array_equal(bits(sb.probs.cpu().numpy()), bits(srv.probs.cpu().numpy()))
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(bits(got[1]), bits(want[1]))
    with pytest.raises(ValueError):
        StreamBatch(pr, dm, S, chunk_size=chunk, heads=bank, stream_heads=[0, 1, 3, 0, 0, 0])
    with pytest.raises(ValueError):
        StreamBatch(pr, dm, S, chunk_size=chunk, stream_heads=[0] * S)
    with pytest.raises(ValueError):
        srv.open(head=3)
    with pytest.raises(ValueError, match="wide"):
        StreamServer(pr, model_of("simple_gru")[1], S, heads=bank)


def test_scan_with_a_head_per_recording_equals_one_scan_per_head(torch):
    from kws_amd.stream import scan
    from kws_amd.transfer import HeadBank
    pr, dm = model_of("simple_cnn")
    heads = stream_heads(dm.embed_size, seed=9)
    bank = named_bank(heads)
    rng = np.random.default_rng(9)
    recs = [pcm_of(rng, n) for n in (9000, 15000, 4001)]
    rec_heads = [2, 0, 1]
    res = scan(pr, dm, recs, chunk_size=700, heads=bank, recording_heads=rec_heads, return_probs=True, tile=8, sensitivity=0.4,
               trigger_level=2)
    assert tuple(res.probs.shape)[2] == 12
    for r, h in enumerate(rec_heads):
        one = scan(pr, dm, [recs[r]], chunk_size=700, heads=HeadBank.from_fits([heads[h]]), return_probs=True, tile=8, sensitivity=0.4,
                   trigger_level=2)
        n, C = one.n_chunks[0], HEAD_CLASSES[h]
        assert n == res.n_chunks[r]
        np.testing.assert_array_equal(bits(res.probs[r, :n, :C].cpu().numpy()), bits(one.probs[0, :n].cpu().numpy()))
        assert not res.probs[r, :n, C:].cpu().numpy().any()
        np.testing.assert_array_equal(res.index[r, :n].cpu().numpy(), one.index[0, :n].cpu().numpy())
        np.testing.assert_array_equal(bits(res.score[r, :n].cpu().numpy()), bits(one.score[0, :n].cpu().numpy()))
        np.testing.assert_array_equal(res.fired[r, :n].cpu().numpy(), one.fired[0, :n].cpu().numpy())
        np.testing.assert_array_equal(res.state[r].cpu().numpy(), one.state[0].cpu().numpy())


def test_score_heads_equals_the_reference_on_three_unequal_folds(torch):
    from kws_amd.transfer import HeadBank, score_heads
    E, N = 128, 5 * T + 7
    emb, heads = hc.make_case(E, (12, 12, 12), N, seed=31)
    rng = np.random.default_rng(31)
    y = rng.integers(0, 12, N)
    y[: N // 2] = np.argmax(ref.logits(emb, heads[0]), axis=1)[: N // 2]       # half the labels agree with head 0: accuracies differ
    perm = rng.permutation(N)
    folds = [np.sort(perm[:T - 3]), np.sort(perm[T - 3:3 * T]), np.sort(perm[3 * T:])]
    want = ref.score(emb, y, heads, folds)
    emb_d = torch.from_numpy(emb).cuda()
    for bank in (HeadBank.from_fits(heads), heads):                            # a bank, or the heads themselves
        acc, loss = score_heads(emb_d, y, bank, folds)
        for h, (hits, n, w_loss) in enumerate(want):
            assert round(acc[h] * n) == hits and abs(acc[h] * n - hits) < 1e-9
            assert abs(loss[h] - w_loss) <= hc.LOSS_RTOL * abs(w_loss), (h, loss[h], w_loss)
    assert len({w[0] / w[1] for w in want}) > 1
    acc, loss = score_heads(emb_d, y, heads, [folds[0], np.zeros(0, np.int64), folds[2]])
    assert np.isnan(acc[1]) and np.isnan(loss[1]) and round(acc[2] * want[2][1]) == want[2][0]
    with pytest.raises(ValueError):
        score_heads(emb_d, np.where(y == 3, 12, y), heads, folds)              # a label outside the head's classes
