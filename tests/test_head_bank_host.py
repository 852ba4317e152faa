"""CPU tests of the head bank (include/kws.h: kws_heads_apply; kws_amd.transfer.HeadBank / plan_bank / score_heads): the argument
checks that run before any device work, the offset planner, the bank's own refusals and the streaming classes' refusals.  The
pointers handed to the library here are never dereferenced: every call must return on its host checks."""
import os
import re

import numpy as np
import pytest

import head_bank_cases as hc
import head_bank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1                        # KWS_ERR_INVALID
P = 0x10000                         # a non-null, 16-byte aligned "pointer"


def base_args():
    """a valid call: emb, N, E, rows, key, key_stride, head_of_key, K, R, weights, weights_count, head_offset, head_classes, H, Cmax,
    logits, probs, pred, stream"""
    return dict(emb=P, N=64, E=128, rows=None, key=P, key_stride=1, head_of_key=None, K=0, R=64, weights=P, weights_count=4096,
                head_offset=P, head_classes=P, H=3, Cmax=12, logits=None, probs=P, pred=None, stream=None)


def call(**change):
    from kws_amd import lib as l
    a = base_args()
    a.update(change)
    rc = l.get_lib().kws_heads_apply(*[a[k] for k in base_args()])
    return rc, l.get_lib().kws_last_error().decode()


BAD = [("E=0", dict(E=0)), ("E=2", dict(E=2)), ("E=6", dict(E=6)), ("E=132", dict(E=132)), ("N<0", dict(N=-1)), ("R<0", dict(R=-1)),
       ("H=0", dict(H=0)), ("Cmax=1", dict(Cmax=1)), ("Cmax=257", dict(Cmax=257)), ("key_stride=0", dict(key_stride=0)),
       ("emb", dict(emb=None)), ("key", dict(key=None)), ("weights", dict(weights=None)), ("head_offset", dict(head_offset=None)),
       ("head_classes", dict(head_classes=None)), ("K=0 with head_of_key", dict(head_of_key=P, K=0)),
       ("no output", dict(logits=None, probs=None, pred=None)), ("R > N without rows", dict(R=65)),
       ("weights_count<0", dict(weights_count=-1)), ("emb misaligned", dict(emb=P + 4))]


@pytest.mark.parametrize("name,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_return_before_any_device_work(name, change):
    rc, msg = call(**change)
    assert rc == INVALID and msg.startswith("heads apply:"), (name, rc, msg)


def test_zero_rows_is_ok_and_touches_nothing():
    assert call(R=0)[0] == 0
    assert call(R=0, N=0)[0] == 0
    assert call(R=0, rows=P, head_of_key=P, K=5, key_stride=8)[0] == 0


def test_header_constants_match_the_library_and_the_case_table():
    from kws_amd import lib as l
    from kws_amd import transfer as tr
    text = open(os.path.join(ROOT, "include", "kws.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (KWS_HEADS_[A-Z_]+) (\d+)", text)}
    assert consts == {"KWS_HEADS_MAX_CLASSES": l.HEADS_MAX_CLASSES, "KWS_HEADS_TILE_ROWS": l.HEADS_TILE_ROWS}
    assert hc.T == l.HEADS_TILE_ROWS
    limits = [tr.max_classes(E) for E in range(4, 129, 4)]            # every E kws_head_fit takes
    assert max(limits) == l.HEADS_MAX_CLASSES and min(limits) >= 2    # every head it can train can be banked
    assert {E: tr.max_classes(E) for E in hc.EMBED_SIZES} == hc.MAX_CLASSES


def test_plan_bank_offsets_and_alignment():
    from kws_amd.transfer import plan_bank
    off, count = plan_bank([2, 3, 64, 5], 128)
    sizes = [129 * c for c in (2, 3, 64, 5)]
    assert off.dtype == np.int64 and off[0] == 0 and all(o % 4 == 0 for o in off) and count % 4 == 0
    for i in range(4):
        end = off[i + 1] if i < 3 else count
        assert off[i] + sizes[i] <= end < off[i] + sizes[i] + 4       # room for the head, less than one alignment step wasted
    off, count = plan_bank([3, 3], 4)                                  # 15 floats each: padded to 16
    assert off.tolist() == [0, 16] and count == 32
    off, count = plan_bank([], 48)
    assert off.size == 0 and count == 0
    for bad_E in (0, 2, 6, 132):
        with pytest.raises(ValueError):
            plan_bank([3], bad_E)
    for bad_C in (1, 257):
        with pytest.raises(ValueError):
            plan_bank([bad_C], 4)


def _head(E, C, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((E, C)).astype(np.float32), rng.standard_normal((C,)).astype(np.float32)


def test_head_bank_refusals_and_bookkeeping(tmp_path):
    from kws_amd.transfer import HeadBank
    with pytest.raises(ValueError):
        HeadBank(6, 2, 5, device="cpu")
    with pytest.raises(ValueError):
        HeadBank(48, 0, 5, device="cpu")
    with pytest.raises(ValueError):
        HeadBank(48, 2, 257, device="cpu")
    bank = HeadBank(48, 2, 5, device="cpu")
    assert bank.offsets.tolist() == [0, 248] and bank.count == 496 and len(bank) == 0
    with pytest.raises(ValueError, match="48-wide|48"):
        bank.add(_head(44, 3))                                          # wrong E
    with pytest.raises(ValueError, match="classes"):
        bank.add(_head(48, 6))                                          # C > max_classes
    with pytest.raises(ValueError, match="background"):
        bank.add(_head(48, 3), ["up", "down", "left"])
    with pytest.raises(ValueError, match="names"):
        bank.add(_head(48, 3), ["background", "up"])
    with pytest.raises(ValueError):
        bank.set(2, _head(48, 3))                                       # no such slot
    assert len(bank) == 0 and not bank.weights.numpy().any()            # a refused head leaves nothing behind
    a, b = _head(48, 3, 1), _head(48, 5, 2)
    assert bank.add(a, ["background", "up", "down"], name="alice") == 0 and bank.add(b) == 1
    with pytest.raises(RuntimeError, match="full"):
        bank.add(_head(48, 2))
    w = bank.weights.numpy()
    np.testing.assert_array_equal(w[:147], np.concatenate([a[0].reshape(-1), a[1]]))        # kws_head_fit's layout, unpacked
    np.testing.assert_array_equal(w[248:248 + 245], np.concatenate([b[0].reshape(-1), b[1]]))
    assert bank.head_classes.tolist() == [3, 5] and bank.classes.tolist() == [3, 5]
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    back = HeadBank.load(path, device="cpu")
    np.testing.assert_array_equal(back.weights.numpy(), w)
    assert back.class_names == [["background", "up", "down"], None] and back.classes.tolist() == [3, 5] and back.names == ["alice", None]
    bank.remove(0)
    assert bank.head_classes.tolist() == [0, 5] and len(bank) == 1 and bank.class_names[0] is None
    assert bank.add(_head(48, 2)) == 0                                  # the freed slot
    both = HeadBank.from_fits([a, b], device="cpu")
    assert (both.embed_size, both.capacity, both.max_classes) == (48, 2, 5)


def test_head_map_names_a_head_per_recording(tmp_path):
    import listen
    from kws_amd.transfer import HeadBank
    bank = HeadBank(4, 3, 3, device="cpu")
    bank.set(0, _head(4, 3), name="alice")
    bank.set(2, _head(4, 2), name="bob")
    path = tmp_path / "map.txt"
    path.write_text("# recording head\na.wav bob\nsub/b.wav 0   # by id\n\nc.wav alice\n")
    assert listen.parse_head_map(str(path), bank) == {"a.wav": 2, "b.wav": 0, "c.wav": 0}
    for bad in ("a.wav carol\n", "a.wav 1\n", "a.wav 3\n", "a.wav\n"):     # no such name, an empty slot, no such slot, a field short
        path.write_text(bad)
        with pytest.raises(ValueError):
            listen.parse_head_map(str(path), bank)
    labels = tmp_path / "labels.txt"
    labels.write_text("a.wav up 0.5 1.0\nb.wav go 0.1 0.2\n")
    names = {"a.wav": ["background", "up"], "b.wav": ["background", "stop", "go"]}
    assert listen.parse_labels(str(labels), names.get, 1000) == {"a.wav": [(1, 500, 1000)], "b.wav": [(2, 100, 200)]}


def test_a_host_bank_is_never_applied():
    import torch
    from kws_amd.transfer import HeadBank, score_heads
    bank = HeadBank.from_fits([_head(4, 3)], device="cpu")
    emb = torch.zeros((8, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="CUDA"):
        bank.apply(emb, [0] * 8)
    with pytest.raises(ValueError):
        score_heads(emb, np.zeros(8, np.int64), bank, [np.arange(8)])


def test_streaming_refusals_come_before_the_device():
    """heads with quantized, a bank of another embedding width, and head ids outside the bank: ValueError on the host"""
    from kws_amd import stream
    from kws_amd.transfer import HeadBank
    bank = HeadBank.from_fits([_head(48, 3)], device="cpu")
    model = type("M", (), {"embed_size": 128, "spec": type("S", (), {"model_type": "simple_cnn"})()})()
    with pytest.raises(ValueError, match="128"):
        stream._check_heads(model, None, bank)
    with pytest.raises(ValueError, match="quantized"):
        stream._check_heads(model, object(), bank)
    stream._check_heads(model, object(), None)                         # no bank: nothing to refuse
    assert stream._head_ids(bank, None, 3, "stream_heads").tolist() == [0, 0, 0]
    for bad in ([0, 1, 0], [0, -1, 0], [0, 0], [0.5, 0, 0]):
        with pytest.raises(ValueError):
            stream._head_ids(bank, bad, 3, "stream_heads")
    with pytest.raises(ValueError, match="HeadBank"):
        stream._head_ids(None, [0], 1, "head")


def test_reference_and_cases_hold_together():
    """the case builders keep their promises: logits within the limit, the pairs' runs around the tile, distinct batches distinct"""
    T = hc.T
    for case in hc.logit_cases():
        emb, heads = hc.make_case(case[0], case[1], 4 * T + 1, seed=1)
        assert all(np.abs(ref.logits(emb, h)).max() <= hc.LOGIT_LIMIT for h in heads)
    rows, heads = hc.independence_pairs(8)
    runs = [int((heads == h).sum()) for h in range(8)]
    assert runs == [T - 1, T + 1, 2 * T, 1, 1, 1, 1, 1] and rows.tolist() == list(range(4 * T + 5))
    seen = np.concatenate(hc.distinct_batches(heads))
    assert sorted(seen.tolist()) == list(range(heads.size))
    assert all(len(set(heads[b].tolist())) == len(b) for b in hc.distinct_batches(heads))
    lg, bd, pr, pred = ref.apply(np.ones((2, 4)), [None, (np.ones((4, 3)), np.array([0.0, 1.0, 1.0]))], [1, 0, 1, 2], 5, rows=[0, 1, 2, 1])
    assert pred.tolist() == [1, -1, -1, -1] and not lg[1:].any() and not pr[:, 3:].any() and abs(pr[0].sum() - 1) < 1e-12
