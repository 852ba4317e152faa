"""The case table of tests/test_lite_maps_gpu.py is sound -- checked on the float64 oracle alone, no device involved: the stated geometry
of every map follows from the restated rules, the arg-max masks stay under their caps, and the comparison can see what it is for (an
oracle that pads stride-2 convolutions on the other side moves the probabilities of exactly the maps meant to catch that, by far more
than the device test's tolerance)."""
import numpy as np
import pytest

import lite_map_cases as lc

IDS = [m.name for m in lc.MAPS]


def test_stated_geometry_follows_from_the_restated_rules():
    assert len(set(IDS)) == len(IDS)
    for m in lc.MAPS:
        d = lc.dims(m.nf, m.fs)
        assert (d["H1"], d["W1"]) == m.s1 and (d["H2"], d["W2"]) == m.s2 and (d["H3"], d["W3"]) == m.s3 and d["flat"] == m.flat, m.name
        assert d["H4"] >= 1 and d["W4"] >= 1, m.name
        assert lc.front_ok(m.nf, m.fs) == m.front and lc.f16_ok(m.nf, m.fs) == m.f16, m.name
        assert (lc.pad_before(d["H2"], 3, 2), lc.pad_before(d["W2"], 3, 2)) == m.pad3, m.name
        assert not m.f16 or m.front
    # all four placements of depthwise 3's padding reach the fp16 kernel
    assert {m.pad3 for m in lc.MAPS if m.f16} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # each refusal has the one reason its row names
    by = {m.name: lc.dims(m.nf, m.fs) for m in lc.MAPS}
    n2 = lambda d: d["H2"] * d["W2"]
    p3 = lambda d: d["H3"] * d["W3"]
    assert (n2(by["12x44"]), p3(by["12x44"]), by["12x44"]["flat"]) == (33, 12, 384)
    assert n2(by["24x26"]) == 36 and p3(by["24x26"]) <= 12 and by["24x26"]["flat"] <= 256
    assert n2(by["32x20"]) == 40 and p3(by["32x20"]) <= 12 and by["32x20"]["flat"] <= 256
    assert (24 + 2) * (30 + 2) == 832 and not lc.front_ok(24, 30)
    # every limit at its edge on 22 x 30, and one step beyond each is refused
    assert ((22 + 2) * (30 + 2), n2(by["22x30"]), p3(by["22x30"]), by["22x30"]["flat"]) == (768, 35, 12, 256)
    assert not lc.front_ok(22, 32) and not lc.front_ok(29, 20) and not lc.front_ok(30, 2)
    assert lc.front_ok(4, 4) and not lc.f16_ok(4, 4)               # no pooled pixel behind stage 3
    assert lc.f16_ok(30, 20, 48) and not lc.f16_ok(30, 20, 49)
    # the front kernel's LDS: the stated largest, and the value the default map has had all along
    assert lc.front_lds_bytes(30, 20) == 4 * (17 * 12 * 16 + 144 * 17)     # a1 with its halo + d2 (larger than xs + d1)
    assert lc.front_lds_bytes(16, 16) == 4 * (10 * 10 * 16 + 64 * 17)
    front = [m for m in lc.MAPS if m.front]
    assert max(front, key=lambda m: lc.front_lds_bytes(m.nf, m.fs)).name == "32x20"
    assert all(lc.front_lds_bytes(m.nf, m.fs) <= 64 * 1024 for m in front)


def test_batch_edges_on_a_256_cu_part():
    cus = lc.MI355X_CUS
    assert lc.front_waves(cus) == 8 * cus                            # 10.5 KiB per wave: the cap of 8 waves per compute unit holds
    b32, b16 = lc.edge_batch("fp32", cus), lc.edge_batch("fp16", cus)
    assert (b32, b16) == (2049, 4113)
    # fp32: two clips per wave, 1025 waves, the last with one clip
    cpw = lc.clips_per_wave(b32, cus)
    assert cpw == 2 and -(-b32 // cpw) == 1025 and b32 - 1024 * cpw == 1
    # fp16: 258 tiles on 256 blocks -- two blocks run the loop twice -- and one clip in the last tile
    ntile = -(-b16 // 16)
    assert ntile == cus + 2 and b16 - 16 * (ntile - 1) == 1
    for other in (104, 304):                                         # the same properties at any compute-unit count
        assert lc.clips_per_wave(lc.edge_batch("fp32", other), other) == 2 and lc.edge_batch("fp32", other) % 2 == 1
        assert -(-lc.edge_batch("fp16", other) // 16) == other + 2 and lc.edge_batch("fp16", other) % 16 == 1
    # the B = 37 cases: one clip per wave, three tiles with 5 clips in the last
    for m in lc.MAPS:
        assert lc.clips_per_wave(lc.B, cus, m.nf, m.fs) == 1
    assert -(-lc.B // 16) == 3 and lc.B % 16 == 5


def _masked(ref):
    return float((~ref.clear).mean())


@pytest.mark.parametrize("m", lc.MAPS, ids=IDS)
def test_masks_stay_under_their_caps_and_a_swapped_padding_side_shows(m):
    d = lc.dims(m.nf, m.fs)
    even = d["H2"] % 2 == 0 or d["W2"] % 2 == 0
    assert even == (0 in m.pad3)
    for path in lc.paths(m):
        ref = lc.reference(m, path)
        assert ref.want.shape == (lc.B, lc.C) and np.isfinite(ref.want).all()
        assert _masked(ref) <= lc.mask_cap(path), "pick another seed for %s: %d of %d clips masked in %s" % (
            m.name, (~ref.clear).sum(), lc.B, path)
        assert np.unique(ref.want.argmax(-1)).size >= 4          # a centred head: the arg-max is not one class everywhere
        # the device gets exactly the oracle's weights
        assert all(np.array_equal(w, np.asarray(w, np.float32)) for w in ref.om.get_weights())
        moved = float(np.abs(lc.swapped_padding_probs(ref.om, ref.x) - ref.want).max())
        tol = lc.TOL_FP16 if path == "fp16" else lc.TOL_FP32
        print("%s %s: masked %d of %d, swapped padding moves a probability by %.3g" % (m.name, path, (~ref.clear).sum(), lc.B, moved))
        if even:
            assert moved > lc.MUTATION_FACTOR * tol, (m.name, path, moved)
        else:
            assert moved == 0.0, (m.name, path, moved)
        # and the oracle is back to TF's rule
        assert np.array_equal(ref.om.predict(ref.x.astype(np.float64)), ref.want)


@pytest.mark.parametrize("path", lc.EDGES)
def test_batch_edge_masks_stay_under_their_caps(path):
    m = lc.MAP[lc.EDGE_MAP]
    ref = lc.reference(m, path, lc.edge_batch(path, lc.MI355X_CUS))
    assert _masked(ref) <= lc.mask_cap(path), (path, _masked(ref))
    # a larger batch extends a smaller one: the B = 37 case's clips are this one's first
    assert np.array_equal(ref.x[:lc.B], lc.reference(m, path).x)
    np.testing.assert_allclose(ref.want[:lc.B], lc.reference(m, path).want, rtol=0, atol=1e-12)
