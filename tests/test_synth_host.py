"""CPU tests of the streaming-recording synthesis: every refusal of kws_synth_plan / kws_synth_render and of the Python layer is
reported without a device, the numpy restatement tests/synth_ref.py keeps its own invariants, the labels file round-trips through
listen.parse_labels, and listen.py's command line takes --synth_from in place of --input_wav."""
import ctypes

import numpy as np
import pytest

import synth_ref

NAMES = ["background", "up", "down", "left", "right"]


def _good():
    from kws_amd.synth import synth_params
    return synth_params(gap=(10, 50), lead_in=5, clip_cap=200, snr=[10.0], bed_gain=(0.05, 0.2), max_gain=8.0, fade=4, seed=1)


def _plan(p, wav_dtype=0, rows=4, stride=200, M=4, R=2, max_events=8, position_base=0):
    from kws_amd import lib as l
    return l.get_lib().kws_synth_plan(None, ctypes.byref(p), None, wav_dtype, rows, stride, None, None, M, None, R, max_events, position_base,
                                      None, None, None)


def _render(wav_dtype=0, rows=4, stride=200, max_events=8, R=2, max_len=1000, fade=0, out_dtype=1, out_stride=1000):
    from kws_amd import lib as l
    return l.get_lib().kws_synth_render(None, None, wav_dtype, rows, stride, None, None, max_events, None, R, max_len, fade, None, out_dtype,
                                        out_stride, None)


@pytest.mark.parametrize("field, value", [("gap_lo", -1), ("gap_hi", 9), ("n_snr", -1), ("n_snr", 17), ("clip_cap", 0), ("max_gain", 0.0),
                                          ("max_gain", -1.0), ("fade", -1), ("bed_gain_hi", 0.01), ("lead_in", -1)])
def test_plan_refuses_bad_parameters_without_a_device(field, value):
    from kws_amd import lib as l
    p = _good()
    setattr(p, field, value)
    assert _plan(p) == l.ERR_INVALID
    assert l.get_lib().kws_last_error()


@pytest.mark.parametrize("kw, code", [(dict(max_events=0), -1), (dict(max_events=4097), -1), (dict(wav_dtype=2), -1), (dict(R=-1), -1),
                                      (dict(position_base=-1), -1), (dict(stride=-1), -1), (dict(stride=2 ** 31), -2),
                                      (dict(rows=0, M=0), -1), (dict(M=0), -1)])
def test_plan_refuses_bad_shapes_without_a_device(kw, code):
    from kws_amd import lib as l
    assert _plan(_good(), **kw) == code
    assert l.get_lib().kws_last_error()
    assert l.get_lib().kws_synth_plan(None, None, None, 0, 4, 200, None, None, 4, None, 2, 8, 0, None, None, None) == l.ERR_INVALID


@pytest.mark.parametrize("kw, code", [(dict(max_events=0), -1), (dict(max_events=4097), -1), (dict(fade=-1), -1), (dict(wav_dtype=3), -1),
                                      (dict(out_dtype=2), -1), (dict(out_stride=999), -1), (dict(R=-1), -1), (dict(max_len=-1, out_stride=0), -1),
                                      (dict(max_len=2 ** 31, out_stride=2 ** 31), -2), (dict(stride=2 ** 31), -2)])
def test_render_refuses_without_a_device(kw, code):
    from kws_amd import lib as l
    assert _render(**kw) == code
    assert l.get_lib().kws_last_error()


def test_no_recordings_do_nothing_and_need_no_device():
    assert _plan(_good(), R=0) == 0
    assert _render(R=0) == 0


def test_record_layouts_match_ctypes():
    from kws_amd import lib as l
    from kws_amd.synth import EVENT_DTYPE, MAX_EVENTS, REC_DTYPE
    assert ctypes.sizeof(l.KwsSynthParams) == 112 and REC_DTYPE.itemsize == 16 and EVENT_DTYPE.itemsize == 32 and MAX_EVENTS == 4096


def test_python_layer_refuses_on_the_host():
    from kws_amd.synth import check_plan, synth_params, synthesize
    for kw in (dict(gap=(-1, 5)), dict(gap=(9, 5)), dict(lead_in=-1), dict(clip_cap=0), dict(snr=[1.0] * 17), dict(snr=[float("nan")]),
               dict(bed_gain=(0.3, 0.1)), dict(max_gain=0), dict(fade=-1)):
        with pytest.raises(ValueError):
            synth_params(**kw)
    clips, labels = np.zeros((3, 100), np.float32), [0, 1, 2]
    for kw in (dict(out_dtype="int8"), dict(position_base=-1), dict(seconds=2.0 ** 31 / 16000), dict(max_events=0), dict(max_events=4097),
               dict(pick=[3]), dict(pick=[]), dict(plan=[[(0, 10), (1, 50)]], seconds=[1.0]),            # overlap: 10 + 100 > 50
               dict(plan=[[(1, 200), (0, 10)]], seconds=[1.0]),                                           # unsorted
               dict(plan=[[(0, 15950)]], seconds=[1.0]),                                                  # past the end
               dict(plan=[[(3, 0)]], seconds=[1.0]),                                                      # no such row
               dict(plan=[[], []], seconds=[1.0])):
        with pytest.raises(ValueError):
            synthesize(clips, labels, sample_rate=16000, clip_cap=16000, **kw)
    with pytest.raises(ValueError):
        synthesize(clips, [0, 1], sample_rate=16000, clip_cap=16000)
    assert check_plan([[(0, 0), (1, 100, 0.5)]], [200], 3, [100, 100, 100]) == [[(0, 0, 1.0), (1, 100, 0.5)]]        # touching, ends at N


@pytest.fixture(scope="module")
def ref_case():
    rng = np.random.default_rng(11)
    clips = rng.uniform(-0.5, 0.5, (7, 200)).astype(np.float32)
    valid = rng.integers(50, 201, 7)
    noise = [rng.uniform(-0.3, 0.3, n).astype(np.float32) for n in (37, 5000)]
    return clips, valid, noise


def test_reference_invariants(ref_case):
    clips, valid, noise = ref_case
    lengths = [20000, 3000, 40, 0]
    kw = dict(gap_lo=10, gap_hi=50, lead_in=7, clip_cap=180, snr_db=(5.0, 20.0), bed_gain=(0.05, 0.2), seed=3, noise=noise)
    rec, ev = synth_ref.plan(clips, valid, lengths, 130, **kw)
    assert rec[0][3] > 64 and rec[2][3] == 0 and rec[3][3] == 0
    for r, N in enumerate(lengths):
        n = rec[r][3]
        placed = ev[r][:n]
        assert all(e == synth_ref.EMPTY for e in ev[r][n:])
        starts = [e[1] for e in placed]
        assert starts == sorted(starts) and all(e[1] + e[2] <= N for e in placed)
        assert all(b[1] - (a[1] + a[2]) >= 10 for a, b in zip(placed, placed[1:]))                       # the gap_lo between two clips
        assert all(50 <= e[2] <= 180 and 0 < e[4] <= 8.0 for e in placed)
        assert 0 <= rec[r][0] < 2 and 0 <= rec[r][1] < len(noise[rec[r][0]]) and 0.05 <= rec[r][2] <= 0.2
    # a larger max_events changes no earlier draw; the same seed gives the same plan
    rec2, ev2 = synth_ref.plan(clips, valid, lengths, 200, **kw)
    assert [e[:130] for e in ev2] == ev and [r[:3] for r in rec2] == [r[:3] for r in rec]
    assert synth_ref.plan(clips, valid, lengths, 130, **kw)[1] == ev
    # a shard planned at its own position is the shard of the whole
    rec3, ev3 = synth_ref.plan(clips, valid, lengths[1:3], 130, position_base=1, **kw)
    assert ev3 == ev[1:3] and rec3 == rec[1:3]
    # fewer slots than fit: every slot is placed
    assert synth_ref.plan(clips, valid, [20000], 5, **kw)[0][0][3] == 5


def test_reference_render_and_int16(ref_case):
    clips, valid, noise = ref_case
    rec = [(0, 30, np.float32(0.1), 2), (-1, 0, np.float32(0), 0)]
    ev = [[(2, 0, 60, 0.0, 1.5), (3, 100, 50, 0.0, 40.0)], []]
    out = synth_ref.render(clips, rec, ev, [150, 90], 160, fade=4, noise=noise)
    assert out.shape == (2, 160) and not out[0, 150:].any() and not out[1].any()
    bed = np.float32(0.1) * noise[0][(30 + np.arange(150)) % 37]
    np.testing.assert_array_equal(out[0, 60:100], bed[60:100])                                           # between the events: the bed alone
    assert out[0, 0] == np.float32(np.float64(np.float32(1.5) * np.float32(0.2)) * np.float64(clips[2, 0]) + np.float64(bed[0]))
    pcm = synth_ref.to_int16(out)
    assert pcm.dtype == np.int16 and pcm.max() == 32767 and np.abs(out).max() > 1.0                      # gain 40 saturates
    assert synth_ref.labelled(ev, rec, [0, 1, 2, 0, 1, 2, 1])[0] == [(2, 0, 60)]                          # row 3 is background


def test_labels_round_trip_through_parse_labels(tmp_path):
    from kws_amd.synth import write_labels
    from listen import parse_labels
    events = [[(1, 16001, 31999), (4, 47999, 63997), (2, 9599999, 9600000)], [], [(3, 1, 2)]]
    names = ["synth_0.wav", "synth_1.wav", "synth_2.wav"]
    path = str(tmp_path / "labels.txt")
    write_labels(path, events, names, NAMES, 16000)
    got = parse_labels(path, NAMES, 16000)
    assert got == {"synth_0.wav": events[0], "synth_2.wav": events[2]}
    write_labels(path, events, names, NAMES, 44100)
    assert parse_labels(path, NAMES, 44100)["synth_0.wav"] == events[0]


def test_listen_arguments_take_synth_from_in_place_of_input_wav(capsys):
    import listen
    args = listen.parse_args(["--model_path", "m.npz", "--sweep", "--synth_from", "data", "--noise_path", "noise", "--synth_recordings", "3",
                              "--synth_seconds", "30", "--synth_gap_s", "0.5,2", "--synth_snr", "5,10", "--synth_seed", "7",
                              "--synth_save_dir", "out"])
    assert args.input_wav is None and args.synth_from == "data" and args.synth_recordings == 3 and args.synth_seconds == 30.0
    assert listen.parse_gap(args.synth_gap_s) == (0.5, 2.0) and args.synth_snr == "5,10" and args.synth_seed == 7 and args.synth_save_dir == "out"
    assert listen.parse_args(["--model_path", "m.npz", "--input_wav", "a.wav"]).synth_from is None
    for argv in (["--model_path", "m.npz", "--sweep"],                                                   # neither input
                 ["--model_path", "m.npz", "--synth_from", "data"],                                      # --synth_from without --sweep
                 ["--model_path", "m.npz", "--sweep", "--synth_from", "data", "--synth_gap_s", "3,1"]):
        with pytest.raises(SystemExit) as e:
            listen.parse_args(argv)
        assert e.value.code == 2
    assert "--input_wav and --synth_from" in capsys.readouterr().err
