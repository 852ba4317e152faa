"""The position-major weight gradient's valid-position lists and block partition (tests/wgrad_pmajor_cases.py, which restates
csrc/kws_cnn_shape.h: wgrad_pm_plan and the block decoding of the kernel in csrc/kws_conv.h), proven on the restatement alone;
tests/test_cnn_shape_host.py holds the C++ plan to it on the host, tests/test_wgrad_pmajor_gpu.py holds
the C++ to the same rule through its results.

Five feature maps (cases.MAPS) and B in 1..70 and 680..1400:
  * every (tap, valid position, 32-clip chunk) belongs to exactly one block and no padding pair to any;
  * the blocks' chunk counts stay within the bound the partition rule implies (stated in the cases module and in the test);
  * the lists equal a brute-force evaluation of sy = oy * stride + kh - pt, sx = ox * stride + kw - pl against the map."""
import collections

import pytest

import wgrad_pmajor_cases as wc

BATCHES = tuple(range(1, 71)) + tuple(range(680, 1401))
PM_MAPS = [m for m in wc.MAPS if wc.applies(*m)]


def test_the_maps_are_what_they_are_here_for():
    assert wc.applies(30, 20) and wc.applies(*wc.ONE_SIDED) and wc.applies(*wc.ODD) and wc.applies(*wc.SIXTEEN)
    assert not wc.applies(*wc.FALLBACK)
    c3, c4 = wc.layers(30, 20)
    assert (c3.H, c3.W, c3.Ho, c3.Wo, c3.pt, c3.pl) == (7, 5, 4, 3, 1, 1)
    # the issue's count on the default map: 70 of the 108 (position, tap) pairs are inside, per tap 6 9 6 / 8 12 8 / 6 9 6
    assert [len(p) for p in wc.plan(c4, 4096).pos] == [6, 9, 6, 8, 12, 8, 6, 9, 6]
    assert wc.plan(c3, 4096).weight == [21, 28, 21] and [len(p) for p in wc.plan(c3, 4096).pos] == [9, 12, 9]
    c3, c4 = wc.layers(*wc.ONE_SIDED)
    assert (c3.H, c3.W, c3.Ho, c3.Wo, c3.pt, c3.pl) == (8, 6, 4, 3, 0, 0)
    assert [len(p) for p in wc.plan(c3, 64).pos] == [12, 12, 9]           # only the last kernel row is padding, at the bottom (sy = 8) ...
    assert wc.plan(c3, 64).weight == [32, 32, 24]                           # ... and only the third tap, in the right column (sx = 6)
    c3, c4 = wc.layers(*wc.ODD)
    assert (c3.H, c3.W, c3.Ho, c3.Wo) == (6, 4, 3, 2)
    c3, c4 = wc.layers(*wc.SIXTEEN)
    assert c4.Ho * c4.Wo == 16
    c3, c4 = wc.layers(*wc.FALLBACK)
    assert c4.Ho * c4.Wo == 20


@pytest.mark.parametrize("nf,fs", PM_MAPS)
def test_lists_equal_brute_force(nf, fs):
    for lay in wc.layers(nf, fs):
        pl = wc.plan(lay, 100)
        for g in range(9 // lay.tpb):
            want = {}
            for oy in range(lay.Ho):
                for ox in range(lay.Wo):
                    mask = 0
                    for t in range(lay.tpb):
                        kh, kw = (g * lay.tpb + t) // 3, (g * lay.tpb + t) % 3
                        sy, sx = oy * lay.stride + kh - lay.pt, ox * lay.stride + kw - lay.pl
                        if 0 <= sy < lay.H and 0 <= sx < lay.W:
                            mask |= 1 << t
                    if mask:
                        want[oy * lay.Wo + ox] = mask
            assert dict(zip(pl.pos[g], pl.taps[g])) == want
            assert pl.pos[g] == sorted(pl.pos[g]) and len(pl.pos[g]) <= 16 and all(p < 16 and m < 16 for p, m in zip(pl.pos[g], pl.taps[g]))
            assert pl.weight[g] == sum(bin(m).count("1") for m in want.values())


@pytest.mark.parametrize("nf,fs", PM_MAPS)
def test_every_valid_chunk_has_one_block_and_no_padding_pair_has_any(nf, fs):
    for lay in wc.layers(nf, fs):
        for B in BATCHES:
            pl = wc.plan(lay, B)
            assert 8 <= wc.grid(pl) <= 8 * wc.MAX_SLOTS and pl.slot0[-1] >= sum(1 for w in pl.weight if w)
            seen = collections.Counter()
            for bid in range(wc.grid(pl)):
                g, items = wc.block_items(lay, pl, B, bid)
                for cc, p, mask in items:
                    for t in range(lay.tpb):
                        if mask >> t & 1:
                            seen[(g * lay.tpb + t, p, cc)] += 1
            nclip = (B + 31) // 32
            want = {(tap, p, cc) for tap in range(9) for p in range(lay.Ho * lay.Wo) if wc.inside(lay, tap, p) for cc in range(nclip)}
            assert set(seen) == want and all(n == 1 for n in seen.values()), (lay.name, B)


@pytest.mark.parametrize("nf,fs", PM_MAPS)
def test_chunk_counts_stay_within_the_rules_bound(nf, fs):
    """Within one (XCD, group) the blocks differ by at most one chunk; the XCDs' clip ranges differ by at most one chunk; a group's
    slots are within one of its exact share S w / sum w (when that is at least one), so a block of group g runs at most
    ceil(n_g NCx / floor(share_g)) chunks in an XCD with NCx clip chunks."""
    for lay in wc.layers(nf, fs):
        for B in BATCHES:
            pl = wc.plan(lay, B)
            S, wsum = pl.slot0[-1], sum(pl.weight)
            per = collections.defaultdict(list)
            for bid in range(wc.grid(pl)):
                g, items = wc.block_items(lay, pl, B, bid)
                per[(bid & 7, g)].append(len(items))
            nclip = (B + 31) // 32
            ncx = [(x + 1) * nclip // 8 - x * nclip // 8 for x in range(8)]
            assert max(ncx) - min(ncx) <= 1 and sum(ncx) == nclip
            for g, w in enumerate(pl.weight):
                n = pl.slot0[g + 1] - pl.slot0[g]
                assert (n == 0) == (w == 0)
                if w and S * w >= wsum:
                    assert abs(n * wsum - S * w) < wsum, (lay.name, B, g, n, S)
                for x in range(8):
                    counts = per[(x, g)]
                    assert len(counts) == n and sum(counts) == ncx[x] * len(pl.pos[g])
                    if counts:
                        assert max(counts) - min(counts) <= 1
                        if S * w >= wsum:
                            assert max(counts) <= -(-len(pl.pos[g]) * ncx[x] // (S * w // wsum))


def test_the_gpu_cases_batches():
    c3, c4 = wc.layers(30, 20)
    assert wc.full_round_batch(c4) == wc.B_FULL
    pl = wc.plan(c4, wc.B_UNEQUAL)
    counts = {len(wc.block_items(c4, pl, wc.B_UNEQUAL, b)[1]) for b in range(wc.grid(pl))}
    assert wc.grid(pl) == 8 * wc.MAX_SLOTS and len(counts) > 1 and min(counts) >= 1
    print("conv4 at B = %d: chunk counts %s" % (wc.B_UNEQUAL, sorted(counts)))
    assert wc.B_UNEQUAL % 32 == 23
    # at B = 4096 (the benchmark's batch) no block of the round runs more than the even share of 70 * 128 chunks, rounded up
    pl = wc.plan(c4, 4096)
    counts = [len(wc.block_items(c4, pl, 4096, b)[1]) for b in range(wc.grid(pl))]
    print("conv4 at B = 4096: %d blocks, %d..%d chunks" % (len(counts), min(counts), max(counts)))
    assert sum(counts) == 70 * 128 and max(counts) == -(-70 * 128 // 768) and min(counts) >= max(counts) - 2
