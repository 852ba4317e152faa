"""CPU proof of the case table of tests/vad_geometry_cases.py, on the float64 restatement tests/vad_ref.py alone: every geometry
tuple (and what kws_vad_create / kws_vad_info make of the same arguments), every refusal, the window counts and boundary
remainders of the rows, the chunk-edge events that tests/test_vad_geometry_gpu.py relies on, and that no row holds a window within
1e-4 of its threshold.  The library is used for its host-only entry points kws_vad_create, kws_vad_info and kws_vad_windows."""
import numpy as np
import pytest

import vad_geometry_cases as gc
import vad_ref

T = 1024                                             # windows per pass of vad_smooth_kernel's loop
BASE_COUNTS = [0, 0, 1, 2, 5, 62, 63, 64, 126, 127, 300]
CHUNK_COUNTS = [1023, 1024, 1025, 2048, 2049, 2100, 2101, 2102, 2103]


def _events(sm):
    """-> (windows where a smoothed interval begins, windows where one ends)"""
    s = np.concatenate([[0], np.asarray(sm, dtype=np.int64)])
    d = np.diff(s)
    return set(np.nonzero(d == 1)[0].tolist()), set(np.nonzero(d == -1)[0].tolist())


@pytest.mark.parametrize("gid", gc.ALL)
def test_geometry_tuples(gid):
    from kws_amd.vad import Vad
    want = gc.GEOMETRIES[gid][1]
    rate, thr, kw = gc.ref_kwargs(gid)
    assert vad_ref.geometry(rate, **kw) == want
    v = Vad(**gc.vad_kwargs(gid))
    assert (v.window_samples, v.hop_samples, v.bin_lo, v.bin_hi, v.median) == want
    assert v.energy_threshold == thr
    N, H = want[:2]
    for a in gc.recordings(gid):
        assert v.n_windows(a.size) == vad_ref.n_windows(a.size, N, H)
    assert want[3] - want[2] + 1 <= 56 and N == 2 * H and N <= 1024 and (want[4] - 1) // 2 <= 127


def test_the_table_reaches_what_it_is_there_for():
    G = {g: t for g, (_, t) in gc.GEOMETRIES.items()}
    assert G["tiny"][1] == 16 and G["tiny"][3] == G["tiny"][0] // 2                  # one K step; the band ends on the Nyquist bin
    assert G["r3200"][3] == G["r3200"][0] // 2
    assert G["tiny_low"][2] % 2 == 0 and G["r11025"][2] % 2 == 0 and G["even_lo"][2] % 2 == 0
    assert G["r11025"][1] % 16 != 0 and G["r44100"][1] % 2 == 1 and (G["r44100"][1] + 15) // 16 * 16 == 448
    assert G["one_bin"][2] == G["one_bin"][3] and G["full_band"][3] - G["full_band"][2] + 1 == 56
    assert G["n1024"][0] == 1024 and G["median1"][4] == 1 and G["median255"][4] == 255 == G["tiny_m255"][4]


@pytest.mark.parametrize("kw,code,word", gc.REFUSALS, ids=[w.replace(" ", "_") for _, _, w in gc.REFUSALS])
def test_refusals(kw, code, word):
    import kws_amd
    from kws_amd.vad import Vad
    with pytest.raises(kws_amd.KwsError) as e:
        Vad(**kw)
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.mark.parametrize("gid", gc.TABLE)
def test_rows_have_the_window_counts_and_remainders(gid):
    N, H = gc.GEOMETRIES[gid][1][:2]
    buf, lens = gc.packed(gid)
    counts = [vad_ref.n_windows(n, N, H) for n in lens]
    assert counts == BASE_COUNTS + (CHUNK_COUNTS if gid in gc.CHUNKED else [])
    assert lens[0] == 0 and lens[1] == N
    assert {(n - N) % H for n in lens if n > N} == {0, 1, H - 1}
    assert buf.shape == (len(lens), max(lens)) and buf.dtype == np.int16
    ref, _ = gc.reference(gid)
    # the contents: an all-zero row, a zero stretch inside the long row, a DC offset, and a tail tone past every length
    assert not buf[3, :lens[3]].any() and not ref[3]["ratio"].any()
    assert not ref[10]["ratio"][150:168].any() and ref[10]["ratio"][:150].all() and not ref[10]["raw"][150:168].any()
    assert abs(float(buf[9, :lens[9]].mean()) - 1000.0) < 50.0
    for r, n in enumerate(lens):
        if n < buf.shape[1]:
            assert np.abs(buf[r, n:].astype(np.int64)).max() > 15000 or buf.shape[1] - n < N // 4
    if gid != "thr0" and gc.GEOMETRIES[gid][1][4] <= 25:
        assert len(ref[10]["intervals"]) == 3 and len(ref[9]["intervals"]) == 2
        assert ref[8]["smoothed"][-1] == 1 and len(ref[8]["intervals"]) == 1          # the open interval is dropped


@pytest.mark.parametrize("gid", gc.ALL)
def test_no_window_within_1e_4_of_the_threshold(gid):
    """tests/test_vad_geometry_gpu.py may set aside at most 0.5 % of a geometry's windows as near-ties: at 1e-4, the ceiling of
    every bound, none is.  The float32 restatement's error is printed beside the bound (-s)."""
    _, thr, _ = gc.ref_kwargs(gid)
    ref, _ = gc.reference(gid)
    total = sum(d["ratio"].size for d in ref)
    near = sum(int(gc.near(d["ratio"], thr, gc.NEAR_WIDTH).sum()) for d in ref)
    print("%s: %d windows, %d within %.0e of %.1f; float32 restatement max |ratio - float64 ratio| = %.3e, measured %.3e, bound %.3e"
          % (gid, total, near, gc.NEAR_WIDTH, thr, gc.f32_error(gid), gc.MEASURED_RATIO_ERR[gid], gc.RATIO_BOUND[gid]))
    assert total >= 750 and near == 0
    assert gc.RATIO_BOUND[gid] == 4 * gc.MEASURED_RATIO_ERR[gid] and 0.0 < gc.RATIO_BOUND[gid] <= gc.CEILING == gc.NEAR_WIDTH
    assert gc.f32_error(gid) <= gc.CEILING


def test_threshold_zero_rows():
    ref, _ = gc.reference("thr0")
    for a, d in zip(gc.recordings("thr0"), ref):
        N, H = 320, 160
        allzero = np.array([not a[w * H:w * H + N].any() for w in range(d["ratio"].size)], dtype=bool)
        assert np.array_equal(d["ratio"] == 0.0, allzero) and np.array_equal(d["raw"], (~allzero).astype(np.uint8))
    assert ref[10]["intervals"] == [(0, 150 * 160)] and ref[10]["smoothed"][-1] == 1


@pytest.mark.parametrize("gid", gc.CHUNKED)
def test_chunk_rows_cross_the_1024_window_edges(gid):
    H = gc.GEOMETRIES[gid][1][1]
    ref, _ = gc.reference(gid)
    rows = ref[len(BASE_COUNTS):]
    assert [d["ratio"].size for d in rows] == CHUNK_COUNTS
    ev = [_events(d["smoothed"]) for d in rows]
    iv = [[(b // H, e // H) for b, e in d["intervals"]] for d in rows]
    for edge in (T, 2 * T):                                            # an interval open across the edge
        assert any(b < edge < e for v in iv for b, e in v), edge
    for w in (T, T - 1):
        assert any(w in b for b, _ in ev), "no begin at window %d" % w
    for w in (T, T + 1, 2 * T):
        assert any(w in e for _, e in ev), "no end at window %d" % w
    # still open at the last window, begun in an earlier chunk: dropped
    assert any(d["smoothed"][-1] == 1 and max(b) // T < (d["smoothed"].size - 1) // T and max(b) > max(e | {0})
               for d, (b, e) in zip(rows, ev))
    # an open one that begins in the last window's own chunk, and a last window that is the 1023rd / 1024th / 1025th
    assert rows[0]["smoothed"][-1] == 1 and rows[2]["smoothed"][-1] == 1 and rows[1]["smoothed"][-1] == 0
    # intervals in all three chunks: span = (first begin of chunk 0, last end of chunk 2)
    d, v = rows[7], iv[7]
    assert any(e < T for _, e in v) and any(T <= b and e < 2 * T or b < T <= e < 2 * T for b, e in v) and any(e >= 2 * T for _, e in v)
    assert d["span"] == (v[0][0] * H, v[-1][1] * H) and v[0][0] < T and v[-1][1] >= 2 * T
    assert d["smoothed"][-1] == 1 and len(v) == 3                      # and a fourth, open at the end, that is not counted
    # short bursts whose raw flags start on the first window of a chunk: only the zeros BEFORE the edge vote them out
    d = rows[8]
    for edge in (T, 2 * T):
        assert d["raw"][edge:edge + 6].all() and not d["raw"][edge - 12:edge].any() and not d["smoothed"][edge - 30:edge + 30].any()
    assert iv[8] == [(299, 500)]


def test_alternating_bursts_number_events_across_chunks():
    ref, _ = gc.reference("tiny_m1")
    d = ref[0]
    assert d["ratio"].size == 2400 and np.array_equal(d["smoothed"], d["raw"])       # median 1
    b, e = _events(d["smoothed"])
    assert len(d["intervals"]) == len(e) > 130
    for c in range(3):
        assert sum(c * T <= w < (c + 1) * T for w in b) >= 40 and sum(c * T <= w < (c + 1) * T for w in e) >= 40
    assert len(d["intervals"]) > 50                                    # the capacity the GPU test runs it at


def test_the_widest_halo_crosses_the_chunk_edge():
    ref, _ = gc.reference("tiny_m255")
    d = ref[0]
    assert 1024 < d["ratio"].size <= 1024 + 127                        # chunk 0's halo is clamped at the recording's end
    assert d["raw"][:T].any() and d["raw"][T:].any() and not d["raw"][T:].all()
    b, e = _events(d["smoothed"])
    assert len(e) == 1 and T < min(e) < T + 127                        # the end's 255 flags lie on both sides of window 1024
    assert not np.array_equal(d["smoothed"], d["raw"])
    assert ref[1]["smoothed"][-1] == 1 and ref[1]["smoothed"][T - 1] == 1 and len(ref[1]["intervals"]) == 1
    d = ref[2]                                                         # raw flags from window 1024 on, none in the 127 before it
    assert d["raw"][T:T + 30].all() and not d["raw"][T - 127:T].any() and not d["smoothed"][T - 127:].any() and len(d["intervals"]) == 1
    # at 16 kHz: rows shorter than the median, ends replicated
    r16, _ = gc.reference("median255")
    assert r16[4]["ratio"].size == 5 and r16[4]["smoothed"].all() and r16[9]["ratio"].size == 127 and not r16[9]["smoothed"].any()
