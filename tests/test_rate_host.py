"""CPU tests of the sample-rate conversion's host half (include/kws.h: kws_rate_bank_*, kws_rate_counts, the argument checks of
kws_rate_convert; kws_amd.rate.RateBank; kws_amd.stream.RaggedPlan with per-slot sample rates) against tests/rate_ref.py, the numpy
restatement of the definition in include/kws.h."""
import ctypes
import math

import numpy as np
import pytest

import rate_ref as rr
from test_stream_ragged_host import PositionListener

PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (32000, 16000), (44100, 16000), (48000, 16000), (16000, 8000), (16000, 44100)]
ZS = (4, 16)
BIG = (2 ** 31 + 7, 2 ** 40 + 3, 2 ** 44)


@pytest.fixture(scope="module")
def banks():
    from kws_amd.rate import RateBank
    return {(fi, fo, Z): (RateBank(fi, fo, zero_crossings=Z), rr.Bank(fi, fo, Z)) for fi, fo in PAIRS for Z in ZS}


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("pair", PAIRS)
def test_bank_matches_the_float64_formula(banks, pair, Z):
    bank, ref = banks[pair + (Z,)]
    g = math.gcd(*pair)
    assert (bank.p, bank.q) == (pair[0] // g, pair[1] // g) == (ref.p, ref.q)
    assert bank.taps == ref.K == (Z if bank.p <= bank.q else -(-Z * bank.p // bank.q))
    assert bank.history == 2 * ref.K - 1
    W = bank.weights()
    assert W.shape == (ref.q, 2 * ref.K) and W.dtype == np.float32 and W.nbytes <= 1 << 20
    err = np.abs(W.astype(np.float64) - ref.W64)
    bound = 2.0 ** -24 * np.abs(ref.W64) * (1 + 1e-6) + 1e-15          # one rounding to float32; tests/test_speed_host.py's bound
    assert np.all(err <= bound), float((err / bound).max())
    # zero where s * distance >= Z; the last tap of the left wing is alive at phase 0, so K is no larger than it must be
    s = min(1.0, ref.q / ref.p)
    dead = s * ref.dist / ref.q >= Z
    np.testing.assert_array_equal(dead, ref.dead)
    assert not W[dead].any() and not dead[0, ref.K - 1] and ref.K * ref.q >= Z * max(ref.p, ref.q)
    if Z == 16:                                                         # unit gain at 0 Hz: every phase's weights sum to 1 within the ripple
        assert np.abs(W.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-3


def test_equal_rates_have_no_taps():
    from kws_amd.rate import RateBank
    b = RateBank(16000, 16000)
    assert (b.p, b.q, b.taps, b.history) == (1, 1, 0, 0) and b.weights().shape == (1, 0)
    assert [b.emitted(n) for n in (0, 1, 5)] == [0, 1, 5] == [b.total(n) for n in (0, 1, 5)]
    assert b.counts(7) == (7, 7) and b.max_chunk(1024) == 1024


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("pair", PAIRS)
def test_counts_match_the_brute_force_count(banks, pair, Z):
    bank, ref = banks[pair + (Z,)]
    p, q, K = ref.p, ref.q, ref.K
    for N in range(0, 3 * K + 5):
        want = rr.emitted_brute(N, p, q, K)
        assert bank.counts(N) == (want, -(-N * q // p)) == (bank.emitted(N), bank.total(N)), N
        assert rr.emitted(N, p, q, K) == want
    for N in BIG:
        e, t = bank.counts(N)
        assert e == bank.emitted(N) == -(-(N - K) * q // p) and t == bank.total(N) == -(-N * q // p)
        # the last emitted output has its rightmost tap inside the stream, the next one does not
        assert ((e - 1) * p) // q + K <= N - 1 < (e * p) // q + K
    arr = np.array([0, K, K + 1, 3 * K + 4, 2 ** 31 + 7], np.int64)
    assert list(bank.emitted(arr)) == [bank.emitted(int(n)) for n in arr] and list(bank.total(arr)) == [bank.total(int(n)) for n in arr]


@pytest.mark.parametrize("pair", PAIRS)
def test_per_push_bound_and_max_chunk(banks, pair):
    bank, ref = banks[pair + (16,)]
    p, q = ref.p, ref.q
    rng = np.random.default_rng(p + q)
    for _ in range(200):
        N, ln = int(rng.integers(0, 100000)), int(rng.integers(1, 5000))
        assert 0 <= bank.emitted(N + ln) - bank.emitted(N) <= -(-ln * q // p)
    for chunk in (1, 7, 160, 1024, 4096):
        mc = bank.max_chunk(chunk)
        assert mc == chunk * p // q == rr.max_chunk(chunk, p, q)
        assert -(-mc * q // p) <= chunk < -(-(mc + 1) * q // p)         # the longest push that cannot overfill a chunk
        for N in (0, ref.K, 12345):
            assert bank.emitted(N + mc) - bank.emitted(N) <= chunk


def test_unsupported_and_invalid_pairs():
    from kws_amd import lib as l
    from kws_amd.rate import RateBank
    L = l.get_lib()
    h = ctypes.c_void_p()

    def create(fi, fo, Z=16, beta=8.5, rolloff=0.85):
        return L.kws_rate_bank_create(fi, fo, Z, beta, rolloff, ctypes.byref(h))

    assert create(16001, 16000) == l.ERR_UNSUPPORTED and b"exceeds" in L.kws_last_error() and not h.value
    assert create(96000, 16000) == l.ERR_UNSUPPORTED and b"ratio" in L.kws_last_error()
    assert create(16000, 3999) == l.ERR_UNSUPPORTED
    for args in ((0, 16000), (16000, 0), (-8000, 16000), (16000, -1)):
        assert create(*args) == l.ERR_INVALID and b"positive" in L.kws_last_error()
    for Z in (3, 33, 0, -1):
        assert create(8000, 16000, Z=Z) == l.ERR_INVALID and b"zero_crossings" in L.kws_last_error()
    assert create(8000, 16000, beta=21.0) == l.ERR_INVALID and create(8000, 16000, rolloff=0.0) == l.ERR_INVALID
    assert L.kws_rate_bank_create(8000, 16000, 16, 8.5, 0.85, None) == l.ERR_INVALID
    with pytest.raises(ValueError, match="ratio") as e:
        RateBank(96000, 16000)
    assert e.value.code == l.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="positive"):
        RateBank(0, 16000)
    assert create(64000, 16000) == 0 and create(4000, 16000) == 0                    # the limits themselves are in
    L.kws_rate_bank_destroy(h)
    # every pair among the common rates within the ratio limit fits, a few hundred KiB at the most
    common = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
    worst = 0
    for fi in common:
        for fo in common:
            if 4 * fi >= fo and 4 * fo >= fi:
                worst = max(worst, RateBank(fi, fo).weights().nbytes)
    assert 100 << 10 < worst < 512 << 10


def test_counts_and_convert_check_their_arguments_on_the_host(banks):
    from kws_amd import lib as l
    L = l.get_lib()
    bank = banks[(44100, 16000, 16)][0]
    e = ctypes.c_int64(0)
    assert L.kws_rate_counts(None, 5, ctypes.byref(e), None) == l.ERR_INVALID
    assert L.kws_rate_counts(bank.handle(), -1, ctypes.byref(e), None) == l.ERR_INVALID
    assert L.kws_rate_counts(bank.handle(), 2 ** 44 + 1, ctypes.byref(e), None) == l.ERR_INVALID
    assert L.kws_rate_bank_weights(bank.handle(), None, 10 ** 6) == l.ERR_INVALID
    small = np.zeros(8, np.float32)
    assert L.kws_rate_bank_weights(bank.handle(), small.ctypes.data, small.size) == l.ERR_INVALID and b"room" in L.kws_last_error()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    hs = (ctypes.c_void_p * 1)(bank.handle())

    def convert(banks_=hs, n_banks=1, wav=p, in_stride=64, in_rows=1, table=p, A=1, hist=None, hist_stride=0, hist_rows=0, o16=p, o32=None,
                out_stride=64, out_rows=1, out_width=64):
        return L.kws_rate_convert(banks_, n_banks, wav, in_stride, in_rows, table, A, hist, hist_stride, hist_rows, o16, o32, out_stride,
                                  out_rows, out_width, None)

    cases = [(lambda: convert(A=-1), b"A=-1"), (lambda: convert(n_banks=0), b"banks"), (lambda: convert(n_banks=17), b"banks"),
             (lambda: convert(banks_=None), b"banks"), (lambda: convert(banks_=(ctypes.c_void_p * 1)(None)), b"null"),
             (lambda: convert(table=None), b"null"), (lambda: convert(wav=None), b"null"), (lambda: convert(o16=None), b"null"),
             (lambda: convert(in_stride=0), b"shapes"), (lambda: convert(out_width=65), b"shapes"), (lambda: convert(out_rows=0), b"output rows"),
             (lambda: convert(hist=p, hist_rows=0), b"hist"), (lambda: convert(hist=None, hist_rows=2), b"hist"),
             (lambda: convert(hist=p, hist_rows=2, hist_stride=2 * bank.taps - 2), b"2K - 1")]
    for call, word in cases:
        assert call() == l.ERR_INVALID
        assert word in L.kws_last_error(), (word, L.kws_last_error())
    assert convert(A=0, wav=None, table=None, o16=None) == 0                         # nothing to do, whatever the pointers
    assert convert(out_stride=2 ** 26, out_width=65535 * 512 + 1) == l.ERR_UNSUPPORTED


def test_the_rate_entry_points_are_declared_and_exported():
    import os
    import re
    from kws_amd import lib as l
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "kws.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(kws_rate_[a-z0-9_]+)\s*\(", text)))
    assert names == ["kws_rate_bank_create", "kws_rate_bank_destroy", "kws_rate_bank_info", "kws_rate_bank_weights", "kws_rate_convert",
                     "kws_rate_counts"]
    for n in names:
        assert hasattr(l.get_lib(), n)
    fields = ("BANK", "IN_ROW", "IN_LEN", "N_LO", "N_HI", "OUT_ROW", "FIRST_LO", "FIRST_HI", "COUNT", "HIST_IN", "HIST_OUT", "FLAGS", "FIELDS",
              "RESTART", "FINAL", "MAX_BANKS")
    assert tuple(getattr(l, "RATE_" + k) for k in fields) == tuple(int(re.search(r"KWS_RATE_%s = (\d+)" % k, text).group(1)) for k in fields)


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return np.clip(6000 * np.sin(0.05 * t) + rng.normal(0, 2500, n), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("pair", [(44100, 16000), (8000, 16000), (16000, 8000)])
def test_the_references_own_chunk_invariance(pair):
    ref = rr.Bank(*pair)
    x = _signal(600, pair[0])
    whole, _, _ = rr.convert(x, ref)
    whole = rr.to_int16(whole)
    assert len(whole) == rr.total(600, ref.p, ref.q)
    M = rr.emitted(600, ref.p, ref.q, ref.K)
    rng = np.random.default_rng(1)
    for trial in range(4):
        cuts = []
        while sum(cuts) < 600:
            cuts.append(int(min(600 - sum(cuts), 1 if trial == 0 and sum(cuts) < 3 * ref.K else rng.integers(1, 200))))
        pieces = rr.stream_int16(x, ref, cuts)
        N = 0
        for c, piece in zip(cuts, pieces):
            assert len(piece) == rr.emitted(N + c, ref.p, ref.q, ref.K) - rr.emitted(N, ref.p, ref.q, ref.K)
            N += c
        np.testing.assert_array_equal(np.concatenate(pieces), whole[:M])


def test_a_tone_survives_the_conversion():
    """1 kHz at 44.1 kHz -> 16 kHz against the ideal tone, away from the ends.  The filter itself is within 1e-5 of unit gain there
    (7.4e-6 in the float64 prototype of the design, full scale); rounding the input to int16 adds at most 2^-16 sum |w| per output."""
    ref = rr.Bank(44100, 16000)
    n = np.arange(8000)
    x = np.round(32767 * np.sin(2 * np.pi * 1000.0 * n / 44100.0)).astype(np.int16)
    y, _, _ = rr.convert(x, ref)
    m = np.arange(len(y))
    ideal = (32767 / 32768.0) * np.sin(2 * np.pi * 1000.0 * m / 16000.0)
    mid = slice(100, len(y) - 100)
    bound = 1e-5 + 2.0 ** -16 * np.abs(ref.W64).sum(axis=1).max()
    err = float(np.abs(y[mid] - ideal[mid]).max())
    print("FIGURES | 1 kHz tone 44.1 -> 16 kHz | max error %.3g, bound %.3g" % (err, bound))
    assert err < bound


# ---- RaggedPlan with per-slot sample rates ---------------------------------------------------------------------------------------------
W_, H_, CHUNK = 1024, 512, 1024


def _plan(S):
    from kws_amd.stream import RaggedPlan
    return RaggedPlan(S, CHUNK, W_, H_, sample_rate=16000)


def test_ragged_plan_with_rates_matches_a_per_slot_loop():
    from kws_amd import lib as l
    rates = [8000, None, 44100, 48000, 16000]
    plan = _plan(len(rates))
    slots = [plan.open(sample_rate=r) for r in rates]
    assert slots == list(range(len(rates)))
    refs = [None if r in (None, 16000) else rr.Bank(r, 16000) for r in rates]
    assert [plan.bank[s] is None for s in slots] == [r is None for r in refs]
    listeners = [PositionListener(W_, H_) for _ in rates]
    received = [0] * len(rates)
    rng = np.random.default_rng(7)
    dropped = 0
    for t in range(300):
        if t == 150:                                                   # slot 2 is reopened at another rate: converter and carry restart
            plan.close(2)
            assert plan.open(sample_rate=11025) == 2
            refs[2], listeners[2], received[2] = rr.Bank(11025, 16000), PositionListener(W_, H_), 0
        active = [int(s) for s in rng.permutation(len(rates)) if rng.random() < 0.7] or [0]
        lens = [int(rng.integers(1, (4 if t % 3 == 0 else plan.max_chunk[s]) + 1)) for s in active]
        step = plan.push(active, lens)
        want_emit = []
        for s, n in zip(active, lens):
            ref = refs[s]
            want_emit.append(n if ref is None else rr.emitted(received[s] + n, ref.p, ref.q, ref.K) - rr.emitted(received[s], ref.p, ref.q, ref.K))
        if all(refs[s] is None for s in active):
            assert step.rate is None and step.entries is None and step.A == len(active)
            kept = list(range(len(active)))
        else:
            assert list(step.emitted) == want_emit and step.rate.shape == (len(active), l.RATE_FIELDS) and step.rate.dtype == np.int32
            kept = [a for a, e in enumerate(want_emit) if e > 0]
            assert list(step.entries) == kept
            dropped += len(active) - len(kept)
            for a, (s, n) in enumerate(zip(active, lens)):
                row, ref = step.rate[a], refs[s]
                assert row[l.RATE_IN_ROW] == a and row[l.RATE_IN_LEN] == n and row[l.RATE_COUNT] == want_emit[a]
                assert row[l.RATE_OUT_ROW] == (kept.index(a) if a in kept else -1)
                if ref is None:
                    assert row[l.RATE_BANK] == 0 and row[l.RATE_HIST_IN] == row[l.RATE_HIST_OUT] == -1 and row[l.RATE_FLAGS] == 0
                    assert row[l.RATE_N_LO] == row[l.RATE_FIRST_LO] == 0
                else:
                    assert plan.banks[row[l.RATE_BANK]] is plan.bank[s] and (plan.bank[s].p, plan.bank[s].q) == (ref.p, ref.q)
                    assert row[l.RATE_N_LO] == received[s] and row[l.RATE_N_HI] == 0
                    assert row[l.RATE_FIRST_LO] == rr.emitted(received[s], ref.p, ref.q, ref.K)
                    assert row[l.RATE_FLAGS] == (l.RATE_RESTART if received[s] == 0 else 0)
                    assert {row[l.RATE_HIST_IN], row[l.RATE_HIST_OUT]} == {2 * s, 2 * s + 1}
        assert step.A == len(kept) and step.table.shape == (len(kept), l.RAGGED_FIELDS)
        for i, a in enumerate(kept):
            s = active[a]
            before, fresh = len(listeners[s].window_audio), listeners[s].arrived == 0
            starts = listeners[s].update_vectors(want_emit[a])
            assert list(step.table[i, :5]) == [s, before, want_emit[a], len(starts), int(fresh)]
            assert int(step.n_new[i]) == len(starts) and step.frame_starts(i) == starts
            assert int(step.carry[i]) == len(listeners[s].window_audio) == int(plan.carry[s])
        for s, n in zip(active, lens):
            received[s] += n
            if refs[s] is not None:
                assert int(plan.received[s]) == received[s]
    assert dropped > 10 and all(li.arrived > 3 * W_ for li in listeners)


def test_history_rows_take_turns():
    from kws_amd import lib as l
    plan = _plan(2)
    s = [plan.open(sample_rate=48000), plan.open()]
    seen = []
    for n in (10, 10, 3000, 5):
        step = plan.push(s, [n, 5])
        seen.append((int(step.rate[0, l.RATE_HIST_IN]), int(step.rate[0, l.RATE_HIST_OUT])))
    assert all(a != b and {a, b} == {0, 1} for a, b in seen) and all(x[1] == y[0] for x, y in zip(seen, seen[1:]))


def test_an_over_long_chunk_is_refused_per_slot():
    plan = _plan(3)
    s48, s8, s16 = plan.open(sample_rate=48000), plan.open(sample_rate=8000), plan.open()
    assert list(plan.max_chunk[[s48, s8, s16]]) == [3072, 512, 1024]
    before = (plan.carry.copy(), plan.received.copy(), plan.parity.copy(), plan.reset.copy())
    with pytest.raises(ValueError, match=r"slot 1 exceeds its max_chunk=512"):
        plan.push([s48, s8], [600, 600])
    with pytest.raises(ValueError, match=r"slot 2 exceeds chunk_size=1024"):
        plan.push([s16], [1025])
    with pytest.raises(ValueError, match=r"slot 0 exceeds its max_chunk=3072"):
        plan.push([s48], [3073])
    for a, b in zip(before, (plan.carry, plan.received, plan.parity, plan.reset)):
        np.testing.assert_array_equal(a, b)                             # a refused push changes nothing
    step = plan.push([s48, s8], [3072, 512])                            # the limits themselves are in: at most chunk_size each
    assert step.emitted.max() <= CHUNK and step.A == 2
    with pytest.raises(ValueError, match="ratio"):
        plan.open(sample_rate=96000)
    from kws_amd.stream import RaggedPlan
    with pytest.raises(ValueError, match="sample_rate"):
        RaggedPlan(2, CHUNK, W_, H_).open(sample_rate=8000)


def test_a_plan_without_rates_gives_todays_tables():
    from kws_amd.stream import RaggedPlan
    old, new, same = RaggedPlan(4, CHUNK, W_, H_), _plan(4), _plan(4)
    for plan, kw in ((old, {}), (new, {}), (same, {"sample_rate": 16000})):
        assert [plan.open(**kw) for _ in range(3)] == [0, 1, 2]
    rng = np.random.default_rng(3)
    for t in range(60):
        active = [int(s) for s in rng.permutation(3)[:int(rng.integers(1, 4))]]
        lens = rng.integers(1, CHUNK + 1, len(active))
        steps = [plan.push(active, lens) for plan in (old, new, same)]
        for st in steps[1:]:
            assert st.rate is None and st.entries is None and st.emitted is None
            for name in ("table", "n_new", "carry", "first"):
                np.testing.assert_array_equal(getattr(steps[0], name), getattr(st, name))
    np.testing.assert_array_equal(old.carry, new.carry)
    np.testing.assert_array_equal(old.position, same.position)
