"""GPU tests of the sample-rate conversion (include/kws.h: kws_rate_convert; kws_amd.rate.convert / launch) against tests/rate_ref.py, the
float64 numpy restatement, fed the library's own bank: every float32 sample within the product-and-sum bound 2 (T + 3) 2^-24 A[n] of
tests/test_speed_gpu.py (T products and T sums of float32, each within 2^-24 relative of A[n] = sum |w| |v|; the "+ 3" covers the
conversion of the sample and the rounding of the reference's own float64 sum), exact lengths, zeros past them; the int16 output against
the float32 output of the same call; and the streaming form -- history rows, restart and flush as StreamServer passes them -- against the
one-shot form, bit for bit, however the stream is cut."""
import numpy as np
import pytest

import rate_ref as rr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TILE = 512                                                              # outputs of one block of rate_convert_kernel
TO_16K = (8000, 11025, 44100, 48000, 16000)                             # the last one is p == q
CASES = [(16000, TO_16K, 4), (16000, TO_16K, 16), (8000, (16000,), 4), (8000, (16000,), 16)]
STREAM_PAIRS = [(8000, 16000), (11025, 16000), (44100, 16000), (48000, 16000), (16000, 8000)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bank(fi, fo, Z):
    from kws_amd.rate import bank_for
    return bank_for(fi, fo, zero_crossings=Z), rr.Bank(fi, fo, Z)


def _lengths(ref):
    """1, K, K + 1, 2K - 1, 2K, the inputs of one output tile -1 / +0 / +1 sample, 3000"""
    K = max(ref.K, 2)
    n_tile = -(-TILE * ref.p // ref.q)                                  # the fewest samples that give TILE outputs ...
    assert rr.total(n_tile, ref.p, ref.q) >= TILE > rr.total(n_tile - 1, ref.p, ref.q) - 1
    return [1, K, K + 1, 2 * K - 1, 2 * K, n_tile - 1, n_tile, n_tile + 1, 3000]


def _pcm(rng, n, clip=False):
    if clip:                                                            # full-scale square wave: the overshoot of the filter clips
        return (32767 * np.where((np.arange(n) // 37) % 2, 1, -1)).astype(np.int16)
    t = np.arange(n)
    return np.clip(7000 * np.sin(0.07 * t + 1.0) + rng.normal(0, 3000, n), -32768, 32767).astype(np.int16)


def _batch(target, rates, Z, seed=0):
    """rows of every length at every rate, plus one clipping row per rate: -> (pcm list, rate list, library banks, reference banks)"""
    rng = np.random.default_rng(seed + Z)
    pcm, rate = [], []
    banks = {r: _bank(r, target, Z) for r in rates}
    for r in rates:
        for n in _lengths(banks[r][1]):
            pcm.append(_pcm(rng, n))
            rate.append(r)
        pcm.append(_pcm(rng, 700, clip=True))
        rate.append(r)
    order = rng.permutation(len(pcm))                                   # mixed rates, row by row
    return [pcm[i] for i in order], [rate[i] for i in order], banks


@pytest.mark.parametrize("target,rates,Z", CASES)
def test_convert_matches_the_float64_restatement(torch, target, rates, Z):
    from kws_amd.rate import convert
    pcm, rate, banks = _batch(target, rates, Z)
    out, lens = convert(pcm, rate, target, dtype=np.float32, zero_crossings=Z)
    again, lens2 = convert(pcm, rate, target, dtype=np.float32, zero_crossings=Z)
    assert out.dtype == torch.float32 and out.is_cuda and lens == lens2 and torch.equal(out.view(torch.int32), again.view(torch.int32))
    got = out.cpu().numpy()
    worst, clipped = 0.0, 0
    for r, (x, fi) in enumerate(zip(pcm, rate)):
        bank, ref = banks[fi]
        want = rr.total(len(x), ref.p, ref.q)
        assert lens[r] == want == bank.total(len(x)), (r, fi, len(x))
        assert not got[r, want:].any(), (r, fi, len(x))                 # zeros past the length
        if ref.K == 0:
            np.testing.assert_array_equal(got[r, :want].view(np.int32), (x.astype(np.float32) / np.float32(32768)).view(np.int32))
            continue
        y, A, T = rr.convert(x, ref, W=bank.weights())
        tol = 2.0 * (T + 3) * U * A
        err = np.abs(got[r, :want].astype(np.float64) - y)
        assert np.all(err <= tol), (r, fi, len(x), int(np.argmax(err - tol)), float(err.max()), float(tol.max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        clipped += int(np.abs(y).max() > 1.0)
    print("FIGURES | convert -> %d Hz, Z = %d, %d rows | worst error / bound = %.3g" % (target, Z, len(pcm), worst))
    assert clipped == sum(1 for fi in set(rate) if banks[fi][1].K)      # every converting rate has its clipping row


@pytest.mark.parametrize("target,rates,Z", CASES)
def test_int16_is_the_rounded_float32_of_the_same_call(torch, target, rates, Z):
    from kws_amd import lib as l
    from kws_amd.rate import convert, launch, rate_table
    from kws_amd.stream import _pack_recordings
    pcm, rate, banks = _batch(target, rates, Z, seed=1)
    keys = sorted(set(rate))
    wav, n_in = _pack_recordings(torch, pcm, None, torch.device("cuda"))
    which = [keys.index(r) for r in rate]
    total = [banks[r][0].total(n) for r, n in zip(rate, n_in)]
    R, width = len(pcm), max(total) + 5
    table = torch.from_numpy(rate_table(which, np.arange(R), n_in, 0, np.arange(R), 0, total, flags=l.RATE_FINAL)).cuda()
    o16 = torch.full((R, width), 77, dtype=torch.int16, device="cuda")
    o32 = torch.full((R, width), 77.0, dtype=torch.float32, device="cuda")
    launch([banks[r][0] for r in keys], wav, table, R, out_i16=o16, out_f32=o32, out_width=width - 2)
    i16, f32 = o16.cpu().numpy(), o32.cpu().numpy()
    assert (i16[:, width - 2:] == 77).all() and (f32[:, width - 2:] == 77.0).all()       # nothing past out_width
    np.testing.assert_array_equal(i16[:, :width - 2], rr.to_int16(f32[:, :width - 2]))
    assert (i16 == 32767).any() and (i16 == -32768).any() and np.abs(f32[:, :width - 2]).max() > 1.0   # the clamp was exercised
    for r, n in enumerate(total):
        assert not i16[r, n:width - 2].any() and not f32[r, n:width - 2].any()
        if rate[r] == target:
            np.testing.assert_array_equal(i16[r, :n], pcm[r])          # p == q: bit for bit
    # the public call gives the same int16 samples and lengths
    out, lens = convert(pcm, rate, target, zero_crossings=Z)
    assert out.dtype == torch.int16 and lens == total
    np.testing.assert_array_equal(out.cpu().numpy()[:, :max(total)], i16[:, :max(total)])


def _stream(torch, bank, x, cuts, chunk_rows=4):
    """The stream x through kws_rate_convert push by push, as StreamServer passes a slot: two history rows by turns, restart with the
    first push (the rows hold garbage before it), a final entry without audio that flushes.  -> (per-push int16 outputs, the tail)"""
    from kws_amd import lib as l
    from kws_amd.rate import launch, rate_table
    hist = torch.full((2, max(bank.history, 1)), 1234, dtype=torch.int16, device="cuda")
    xs = torch.from_numpy(x).cuda()
    N, par, pieces = 0, 0, []
    for i, c in enumerate(list(cuts) + [0]):
        final = i == len(cuts)
        lo = bank.emitted(N)
        cnt = (bank.total(N) if final else bank.emitted(N + c)) - lo
        table = rate_table(0, 0, c, N, 0 if cnt else -1, lo, cnt, par, par ^ 1, (l.RATE_RESTART if i == 0 else 0) | (l.RATE_FINAL if final else 0))
        wav = xs[N:N + c].reshape(1, -1) if c else torch.zeros((1, 1), dtype=torch.int16, device="cuda")
        out = torch.full((1, cnt + 3), 77, dtype=torch.int16, device="cuda")
        launch([bank], wav.contiguous(), torch.from_numpy(table).cuda(), 1, out_i16=out, out_width=cnt, hist=hist)
        got = out[0].cpu().numpy()
        assert (got[cnt:] == 77).all()
        pieces.append(got[:cnt])
        N, par = N + c, par ^ 1
        assert sum(len(p) for p in pieces) == (bank.total(N) if final else bank.emitted(N))            # the count after every push is M(N)
    return pieces[:-1], pieces[-1]


@pytest.mark.parametrize("Z", [4, 16])
@pytest.mark.parametrize("pair", STREAM_PAIRS)
def test_any_cutting_of_a_stream_gives_the_one_shot_samples(torch, pair, Z):
    from kws_amd.rate import convert
    bank, ref = _bank(pair[0], pair[1], Z)
    rng = np.random.default_rng(pair[0] + Z)
    n = 3000
    x = _pcm(rng, n)
    x[1500:1600] = _pcm(rng, 100, clip=True)                            # a stretch that clips
    whole, lens = convert([x], pair[0], pair[1], zero_crossings=Z)
    whole = whole[0, :lens[0]].cpu().numpy()
    M = bank.emitted(n)
    assert lens[0] == bank.total(n) == rr.total(n, ref.p, ref.q) and M == rr.emitted(n, ref.p, ref.q, ref.K) and 0 < M < lens[0]
    mc = bank.max_chunk(256)
    ones = [1] * (3 * ref.K)
    cuttings = [ones + [n - len(ones)], [], [n]]
    while sum(cuttings[1]) < n:
        cuttings[1].append(int(min(n - sum(cuttings[1]), rng.integers(1, mc + 1))))
    for cuts in cuttings:
        pieces, tail = _stream(torch, bank, x, cuts)
        N = 0
        for c, piece in zip(cuts, pieces):
            assert len(piece) == rr.emitted(N + c, ref.p, ref.q, ref.K) - rr.emitted(N, ref.p, ref.q, ref.K)
            N += c
        np.testing.assert_array_equal(np.concatenate(pieces), whole[:M])         # identical across the cuttings, and to the one-shot prefix
        np.testing.assert_array_equal(tail, whole[M:])                          # the flush yields the one-shot tail
    assert len(pieces[0]) == M                                                   # the last cutting: one chunk


def test_entries_share_a_launch_and_a_short_chunk_shifts_the_history(torch):
    """two streams of different rates in one launch per push, their chunks shorter than the history: the rows shift"""
    from kws_amd import lib as l
    from kws_amd.rate import convert, launch, rate_table
    banks = [_bank(44100, 16000, 16)[0], _bank(8000, 16000, 16)[0]]
    rng = np.random.default_rng(5)
    xs = [_pcm(rng, 400), _pcm(rng, 400)]
    hist = torch.zeros((4, max(b.history for b in banks)), dtype=torch.int16, device="cuda")
    N, par, got = [0, 0], 0, [[], []]
    step = (7, 5)                                                       # both far below 2K - 1 = 89 and 31
    while N[0] < 400 or N[1] < 400:
        c = [min(step[s], 400 - N[s]) for s in range(2)]
        wav = torch.zeros((2, 8), dtype=torch.int16, device="cuda")
        for s in range(2):
            wav[s, :c[s]] = torch.from_numpy(xs[s][N[s]:N[s] + c[s]]).cuda()
        lo = [banks[s].emitted(N[s]) for s in range(2)]
        cnt = [banks[s].emitted(N[s] + c[s]) - lo[s] for s in range(2)]
        table = rate_table([0, 1], [0, 1], c, N, [0, 1], lo, cnt, [par, 2 + par], [par ^ 1, 2 + (par ^ 1)], l.RATE_RESTART if N[0] == 0 else 0)
        out = torch.zeros((2, 16), dtype=torch.int16, device="cuda")
        launch(banks, wav, torch.from_numpy(table).cuda(), 2, out_i16=out, hist=hist)
        o = out.cpu().numpy()
        for s in range(2):
            got[s].append(o[s, :cnt[s]])
            N[s] += c[s]
        par ^= 1
    h = hist.cpu().numpy()
    for s, rate in enumerate((44100, 8000)):
        whole, lens = convert([xs[s]], rate, 16000)
        np.testing.assert_array_equal(np.concatenate(got[s]), whole[0, :banks[s].emitted(400)].cpu().numpy())
        np.testing.assert_array_equal(h[2 * s + par, :banks[s].history], xs[s][400 - banks[s].history:])   # the current row: the last 2K - 1
