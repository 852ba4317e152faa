"""The case table of the frame-geometry tests (tests/geometry_cases.py) is sound -- checked on the host alone: every row has the frame
count it states, reaches the kernel it names under the restated dispatch rules, hits the job shapes (fpw, jpc, idle waves, segment
tiles) its reason promises, at 256 compute units and at another count; and `kws_amd.stream.scan_plan`, the closed form behind `scan`,
equals the chunk loop it restates at every row and chunk size where hop <= window, and refuses hop > window, where it does not."""
import numpy as np
import pytest

import geometry_cases as gc

IDS = [g.name for g in gc.ROWS]


def test_rows_have_their_stated_frames_and_kernels():
    assert len(set(IDS)) == len(IDS)
    for g in gc.ROWS:
        assert gc.clip_frames(g) == gc.n_features(g) == g.frames, g.name            # kws_featurizer_create accepts it
        pts = gc.mel_points(g)
        assert all(b > a for a, b in zip(pts, pts[1:])) and pts[-1] <= g.n_fft // 2 + 1, g.name
        assert gc.kernel_of(g) == g.kernel, g.name
        assert gc.max_samples(g) % 2 == 0 and gc.stride(g) % 2 == 1, g.name         # rows at an odd stride
        assert gc.window_samples(g) <= gc.max_samples(g)
        p = gc.params(g)
        assert (p.window_samples, p.hop_samples, p.max_samples, p.n_features, p.feature_size) == (
            gc.window_samples(g), gc.hop_samples(g), gc.max_samples(g), g.frames, gc.feature_size(g)), g.name
        lens = gc.base_lengths(g)
        W, M = gc.window_samples(g), gc.max_samples(g)
        assert {0, 1, W - 1, W, M}.issubset(set(lens.tolist())) and (lens > gc.stride(g)).any() and (lens[2] % 2 == 1 and 1 < lens[2] <= M)
        assert sorted(set(gc.batch_index(gc.N_BASE).tolist())) == list(range(gc.N_BASE))
    assert [gc.ROW[n].frames % 3 for n in gc.TUNED] == [2, 2, 1, 0]
    assert gc.ROW["tuned-2"].frames < gc.tail_batch(gc.ROW["tuned-2"]) == 3
    # the default geometry is the tuned kernel's, and each of its conditions alone sends a row elsewhere
    default = gc.Geometry("default", 1.0, 0.064, 0.032, 1024, 20, 20, False, 30, "tuned", "")
    assert gc.kernel_of(default) == "tuned" and gc.kernel_of(default, use_delta=True) == "gen1"
    assert gc.kernel_of(default._replace(hop_t=0.016)) == "gen1" and gc.kernel_of(default._replace(n_filt=40)) == "gen1"
    assert gc.kernel_of(default._replace(window_t=0.025)) == "gen1" and gc.kernel_of(default._replace(n_fft=512)) == "generic"


@pytest.mark.parametrize("cus", [gc.MI355X_CUS, gc.OTHER_CUS])
def test_tuned_batches_hit_their_job_shapes(cus):
    for name in gc.TUNED:
        g = gc.ROW[name]
        bs = gc.tuned_batches(g, cus)
        tb = min(g.frames, 3)
        assert gc.v3_job_shape(g.frames, 1, cus)[:2] == (tb, -(-g.frames // tb)), name
        fpw, jpc, rounds = gc.v3_job_shape(g.frames, bs["tail"], cus)
        assert fpw == tb and rounds == 1 and bs["tail"] * jpc <= gc.v3_waves(cus), name
        assert gc.v3_waves(cus) < (bs["tail"] + 1) * jpc or bs["tail"] == gc.MAX_CLIPS, name
        if name == "tuned-2":
            assert bs["odd"] is None and bs["whole"] is None and bs["tail"] == gc.MAX_CLIPS
            continue
        if bs["whole"] is None:         # more waves than 256 compute units have: 61 frames per job may not pay within MAX_CLIPS clips
            assert cus != gc.MI355X_CUS and all(gc.v3_job_shape(g.frames, b, cus)[0] < g.frames for b in range(2, gc.MAX_CLIPS + 1, 7)), name
        else:
            fpw, jpc, rounds = gc.v3_job_shape(g.frames, bs["whole"], cus)
            assert (fpw, jpc) == (g.frames, 1), name
        if name != "tuned-45":          # 14 % 3 and 61 % 3 are not 0: the clip's last tail batch is partly filled at any fpw
            fpw, jpc, rounds = gc.v3_job_shape(g.frames, bs["odd"], cus)
            assert 3 < fpw < g.frames and fpw % 3 and bs["odd"] * -(-g.frames // 3) > gc.v3_waves(cus), name
        assert max(b for b in bs.values() if b) <= gc.MAX_CLIPS
        # the shared-CU form (12 waves per compute unit) deals the same batches differently somewhere
        assert any(gc.v3_job_shape(g.frames, b, cus, shared=True) != gc.v3_job_shape(g.frames, b, cus) for b in bs.values() if b), name
    if cus == gc.MI355X_CUS:
        assert gc.v3_waves(cus) == 4096 and gc.v3_waves(cus, shared=True) == 3072
        assert gc.v3_job_shape(14, 1000, cus)[:2] == (4, 4)
        assert gc.tuned_batches(gc.ROW["tuned-14"], cus) == {"one": 1, "tail": 819, "odd": 820, "whole": 2731}
        # batch invariance is checked across two B that pick different fpw
        for name in gc.TUNED[1:]:
            shapes = {gc.v3_job_shape(gc.ROW[name].frames, b, cus)[0] for b in gc.batches(gc.ROW[name], cus)}
            assert len(shapes) >= 3, name


def test_first_generation_job_shapes_and_idle_waves():
    g = gc.ROW["gen1-9"]
    assert gc.tail_batch(g) == 3 and gc.feat_job_shape(9, 3, False) == (3, 3)
    assert gc.window_eff(g) == 1024 and 2 * gc.hop_samples(g) != 1024              # no half-frame reuse
    assert gc.gen1_grid(4, 3, False) == (3, 3) and gc.gen1_grid(1, 3, False) == (1, 2)
    assert gc.batches(g, gc.MI355X_CUS) == gc.batches(g, gc.OTHER_CUS) == [1, 4]
    # what the suite ran before: 30 frames at B = 2 and 3 with 5 jobs per clip -- never an idle wave
    assert gc.feat_job_shape(30, 1, False) == (6, 5) and all(gc.gen1_grid(B, 5, False)[1] == 0 for B in (2, 3))
    g = gc.ROW["gen1-48"]
    assert gc.tail_batch(g) == 1 and gc.window_eff(g) == 400 and gc.feat_job_shape(48, 1, False) == (10, 5)
    assert gc.gen1_grid(7, 5, False) == (7, 0)
    d = gc.ROW["gen1-48d"]
    assert gc.feat_job_shape(48, gc.tail_batch(d), True) == (10, 5) and gc.gen1_grid(7, 5, True) == (7, 0) and gc.feature_size(d) == 26
    # the segments of kws_featurize_long are clips of 256 frames: 52 per job, the fifth job short
    assert gc.feat_job_shape(gc.LONG_TILE, 1, False) == (52, 5) and gc.LONG_TILE - 4 * 52 == 48
    for cus in (gc.MI355X_CUS, gc.OTHER_CUS):
        for name in ("rad2-48", "rad2-31"):
            assert gc.batches(gc.ROW[name], cus) == [1, 5, cus + 3]


def test_long_rows_take_the_segment_path_on_the_non_tuned_rows():
    for name in gc.LONG_ROWS:
        g = gc.ROW[name]
        assert gc.long_uses_segments(g) and not g.use_delta
        assert gc.long_tile(g, 2 * gc.LONG_TILE + 44) == (gc.LONG_TILE, 3)
        assert gc.long_tile(g, 100) == (100, 1)
    assert not gc.long_uses_segments(gc.ROW["tuned-14"])
    big = gc.ROW["rad2-48"]._replace(n_fft=4096, n_filt=64, n_mfcc=64)            # the LDS rule bites only far from the table
    assert gc.long_tile(big, 1000)[0] == (gc.MAX_LDS - 4 * 4096 * 8 - 1024) // 256 - 4 == 120


def test_stream_rows_and_models():
    assert [gc.stream_model_kind(gc.ROW[n]) for n in gc.STREAM_ROWS] == ["simple_cnn", "simple_gru", "simple_cnn", "simple_cnn", "simple_cnn"]
    for n in gc.STREAM_ROWS:
        g = gc.ROW[n]
        W, H = gc.window_samples(g), gc.hop_samples(g)
        half, c800, odd, big = gc.stream_chunks(g)
        assert half < H and (W + odd) % 2 == 1 and gc.raw_frames(g, big) > g.frames
    assert gc.window_samples(gc.ROW["rad2-48"]) % gc.hop_samples(gc.ROW["rad2-48"]) != 0
    assert gc.hop_samples(gc.ROW["rad2-31"]) > gc.window_samples(gc.ROW["rad2-31"])


def _plan_lengths(g, chunk):
    """recordings that end on / one short of / one past a chunk and a frame boundary, shorter than a window, and of many chunks"""
    W, H = gc.window_samples(g), gc.hop_samples(g)
    out = {1, W - 1, W, W + 1, chunk - 1, chunk, chunk + 1, 7 * chunk + 1, W + 6 * H - 1, W + 6 * H, W + 41 * H + 1}
    out.add(min(23 * chunk - 1, 40000))
    return sorted(n for n in out if n > 0)


@pytest.mark.parametrize("g", gc.ROWS, ids=IDS)
def test_scan_plan_is_the_chunk_loop_at_every_geometry(g):
    from kws_amd.stream import scan_plan
    W, H, F = gc.window_samples(g), gc.hop_samples(g), g.frames
    if H > W:
        for chunk in gc.plan_chunks(g):
            with pytest.raises(ValueError, match="hop"):
                scan_plan(20 * chunk, chunk, W, H, F)
        return
    for chunk in gc.plan_chunks(g):
        for N in _plan_lengths(g, chunk):
            T, n, r, first = scan_plan(N, chunk, W, H, F)
            loop = gc.chunk_loop_rows(g, N, chunk)
            assert T == len(loop) == -(-N // chunk), (N, chunk)
            for k, (made, marks, carry, carry_first) in enumerate(loop):
                assert made == r[k], "N=%d chunk=%d chunk %d: %d rows, plan %d" % (N, chunk, k + 1, made, r[k])
                want = [j * H + 1 if j >= 0 else 0 for j in range(first[k], r[k])]
                assert marks.tolist() == want, (N, chunk, k)
                assert carry == n[k] - r[k] * H and (carry == 0 or carry_first == r[k] * H + 1)
    # the chunk sizes do what they are there for
    _, _, r, _ = scan_plan(40 * (H // 2), H // 2, W, H, F)
    assert any(a == b for a, b in zip(r[2 * W // H + 2:], r[2 * W // H + 3:]))     # pushes that bring no row
    _, _, r, _ = scan_plan(3 * 5000, 5000, W, H, F)
    assert r[1] - r[0] > 1


def test_hop_larger_than_window_is_refused_because_the_closed_form_fails_there():
    """rad2-31 (window 256, hop 512) at chunk 800: a push consumes more samples than it holds, the carry empties (listen.py:105) and the
    next frame starts where the next chunk does, not on a multiple of the hop.  The chunk loop makes 2, 4, 6, 8 rows; rows counted from
    sample 0 would be 2, 3, 5, 6."""
    from kws_amd.stream import scan_plan
    g = gc.ROW["rad2-31"]
    W, H = gc.window_samples(g), gc.hop_samples(g)
    loop = gc.chunk_loop_rows(g, 4 * 800, 800)
    assert [v[0] for v in loop] == [2, 4, 6, 8] and [v[2] for v in loop] == [0, 0, 0, 0]
    assert [gc.raw_frames(g, n) for n in (800, 1600, 2400, 3200)] == [2, 3, 5, 6]
    assert loop[1][1][-1] == 800 + H + 1                                            # row 3 starts at sample 800 + 512, no multiple of 512
    with pytest.raises(ValueError, match="hop"):
        scan_plan(3200, 800, W, H, g.frames)
    assert scan_plan(3200, 800, W, W, g.frames)[2] == [3, 6, 9, 12]              # hop == window is the closed form's edge


def test_oracle_references_are_shared_and_read_only():
    g = gc.ROW["gen1-48d"]
    want = gc.base_features(g)
    assert want is gc.base_features(g) and not want.flags.writeable
    assert want.shape == (gc.N_BASE, 48, 26) and np.isfinite(want).all()
    assert np.array_equal(want[0, :, 0], np.full(48, np.log(np.finfo(float).eps)))   # the empty clip: log floor, exactly
    a = gc.base_clips(g)
    assert a.dtype == np.float32 and np.array_equal(a * 32768, np.round(a * 32768)) and 0.05 < a.std() < 0.15
