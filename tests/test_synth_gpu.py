"""GPU tests of the streaming-recording synthesis (kws_synth_plan, kws_synth_render, kws_amd.synth) against the numpy restatement
tests/synth_ref.py.  Draws, starts, lengths and counts are compared exactly (integers); gains against float64 at rtol 1e-5, the bound
tests/test_augment_gpu.py uses for the noise mix's gain (fp32 lane partials of the clip's power); the render at atol 1e-6 on samples
below amplitude 1, the project's bound for kws_augment_apply (one fused multiply-add per sample on both sides)."""
import numpy as np
import pytest

import synth_ref

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]
RATE = 16000
TILE = 4096                                                       # csrc/kws_synth.hip: kSynthTile


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def store():
    """7 clips of 50..200 samples in rows of 200, row 5 silent; noise segments of 37 and 3000 samples"""
    rng = np.random.default_rng(21)
    clips = rng.uniform(-0.5, 0.5, (7, 200)).astype(np.float32)
    valid = rng.integers(50, 201, 7).astype(np.int32)
    valid[0], valid[6] = 50, 200
    clips[5] = 0.0
    noise = [rng.uniform(-0.3, 0.3, n).astype(np.float32) for n in (37, 3000)]
    for a in (clips, valid):
        a.setflags(write=False)
    return clips, valid, noise


KW = dict(gap_s=(10 / RATE, 50 / RATE), lead_in_s=7 / RATE, bed_gain=(0.05, 0.2), max_gain=8.0, fade_ms=0, sample_rate=RATE, clip_cap=180)
REF = dict(gap_lo=10, gap_hi=50, lead_in=7, clip_cap=180, bed_gain=(0.05, 0.2), max_gain=8.0)


def _edge_lengths(clips, valid, seed, pick):
    """N_0: event 100 ends exactly at N_0; N_1: event 100 would end at N_1 + 1; N_2: too short for any event"""
    _, ev = synth_ref.plan(clips, valid, [10 ** 6] * 2, 130, seed=seed, pick=pick, with_gains=False, **REF)
    ends = [ev[r][100][1] + ev[r][100][2] for r in range(2)]
    return [ends[0], ends[1] - 1, 40]


def _compare_plan(got_rec, got_ev, rec, ev, gains=True):
    for r in range(len(rec)):
        assert (got_rec["segment"][r], got_rec["offset"][r], got_rec["n_events"][r]) == (rec[r][0], rec[r][1], rec[r][3]), r
        np.testing.assert_allclose(got_rec["bed_gain"][r], rec[r][2], rtol=1e-6)
        for name, i in (("row", 0), ("start", 1), ("length", 2)):
            np.testing.assert_array_equal(got_ev[name][r], [e[i] for e in ev[r]], err_msg="%s of recording %d" % (name, r))
        np.testing.assert_array_equal(got_ev["snr_db"][r], np.array([e[3] for e in ev[r]], np.float32))
        if gains:
            np.testing.assert_allclose(got_ev["gain"][r], [e[4] for e in ev[r]], rtol=1e-5, atol=0, err_msg="gain of recording %d" % r)


@pytest.mark.parametrize("pick", [None, [6, 0, 2, 2, 5]])
def test_plan_equals_numpy(torch, store, pick):
    """130 slots and more than 64 placed: the scan's carry between lane groups; the three edges of the fit rule; shards; repeats"""
    from kws_amd.synth import synthesize
    clips, valid, noise = store
    seed = 5
    lens = _edge_lengths(clips, valid, seed, pick)
    rec, ev = synth_ref.plan(clips, valid, lens, 130, snr_db=(5.0, 20.0), seed=seed, pick=pick, noise=noise, **REF)
    assert [r[3] for r in rec] == [101, 100, 0]
    assert ev[0][100][1] + ev[0][100][2] == lens[0] and ev[1][99][1] + ev[1][99][2] < lens[1]
    args = dict(valid_len=valid, noise=noise, snr=[5.0, 20.0], seed=seed, pick=pick, max_events=130, out_dtype="float32", **KW)
    full = synthesize(clips, np.arange(7) % 5, seconds=[n / RATE for n in lens], **args)
    assert full.lengths == lens
    got_rec, got_ev = full.records()
    _compare_plan(got_rec, got_ev, rec, ev)
    # the events listed are the placed clips of a class other than the background (rows 0 and 5 carry class 0)
    assert full.events == synth_ref.labelled(ev, rec, np.arange(7) % 5)
    assert sum(len(e) for e in full.events) > 64
    # the same seed twice is bit-equal, records and samples
    again = synthesize(clips, np.arange(7) % 5, seconds=[n / RATE for n in lens], **args)
    assert torch.equal(again.rec, full.rec) and torch.equal(again.plan, full.plan) and torch.equal(again.wav, full.wav)
    # recordings [1, 3) planned at position_base = 1 are rows 1..2 of the full plan
    shard = synthesize(clips, np.arange(7) % 5, seconds=[n / RATE for n in lens[1:]], position_base=1, **args)
    assert torch.equal(shard.rec, full.rec[1:]) and torch.equal(shard.plan, full.plan[1:])
    # a larger max_events changes no earlier slot
    more = synthesize(clips, np.arange(7) % 5, seconds=[n / RATE for n in lens], **dict(args, max_events=200))
    assert torch.equal(more.plan[:, :130], full.plan) and torch.equal(more.rec, full.rec)


def test_gains_against_float64(torch, store):
    from kws_amd.synth import synthesize
    clips, valid, noise = store
    lens = [20000, 9000]
    labels = np.arange(7) % 5
    args = dict(valid_len=valid, seed=9, max_events=130, out_dtype="float32", **KW)
    for bank, what in (([noise[0]], "a 37-sample segment: every window wraps more than once"), ([noise[1]], "windows that wrap once")):
        rec, ev = synth_ref.plan(clips, valid, lens, 130, snr_db=(0.0, 10.0, 30.0), seed=9, noise=bank, **REF)
        placed = [e for r in range(2) for e in ev[r][:rec[r][3]]]
        L = len(bank[0])
        wraps = [(rec[r][1] + e[1]) % L + e[2] > L for r in range(2) for e in ev[r][:rec[r][3]]]
        assert all(wraps) if L == 37 else (any(wraps) and not all(wraps)), what
        silent = [e for e in placed if e[0] == 5]
        assert silent and all(e[4] == 8.0 for e in silent)                                    # a silent clip takes max_gain
        assert any(0 < e[4] < 8.0 for e in placed)
        got = synthesize(clips, labels, seconds=[n / RATE for n in lens], noise=bank, snr=[0.0, 10.0, 30.0], **args)
        _compare_plan(*got.records(), rec, ev)
    for kw in (dict(noise=noise, snr=None), dict(noise=None, snr=[10.0])):                     # n_snr = 0; no bank
        got_rec, got_ev = synthesize(clips, labels, seconds=[n / RATE for n in lens], **dict(args, **kw)).records()
        for r in range(2):
            n = got_rec["n_events"][r]
            assert n > 30 and (got_ev["gain"][r, :n] == 1.0).all() and (got_ev["gain"][r, n:] == 0.0).all()
        assert (got_rec["segment"] >= 0).all() if kw["noise"] else (got_rec["segment"] == -1).all()


def _render_plan(valid, gain=1.5):
    """-> (lengths, plan, valid_len with row 0 cut to 5 samples).  Recording 0 (10000 samples: three tiles, the last partial): an event at sample 0, one across the first tile boundary, one that
    ends at N; 1 (1000: less than a tile); 2 (5000): 300 events of 5 samples, more than the kernel stages, across a tile boundary; 3: none;
    4: no samples"""
    lens = [10000, 1000, 5000, 3000, 0]
    tiny = [(0, 2000 + 8 * i, gain) for i in range(300)]
    assert tiny[0][1] < TILE < tiny[-1][1] and 10000 % TILE and 1000 < TILE
    plan = [[(6, 0, gain), (6, TILE - 96, 0.7), (2, 8000, gain), (6, 10000 - 200, 1.0)], [(3, 400, gain)], tiny, [], []]
    valid = valid.copy()
    valid[0] = 5
    return lens, plan, valid


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("fade_ms", [0, 10])
def test_render_equals_the_reference(torch, store, dtype, fade_ms):
    """fade_ms = 10 is 160 samples: longer than half of every clip"""
    from kws_amd.synth import synthesize
    clips, valid, noise = store
    if dtype == "int16":
        clips = synth_ref.to_int16(clips)
    lens, plan, valid = _render_plan(valid)
    kw = dict(KW, fade_ms=fade_ms, clip_cap=200)
    got = synthesize(clips, np.arange(7) % 5, valid_len=valid, noise=noise, seconds=[n / RATE for n in lens], plan=plan, seed=2,
                     out_dtype="float32", **kw)
    rec, ev = got.records()
    assert [int(n) for n in rec["n_events"]] == [4, 1, 300, 0, 0] and set(rec["segment"].tolist()) <= {0, 1}
    ref_rec = [(int(r["segment"]), int(r["offset"]), r["bed_gain"], int(r["n_events"])) for r in rec]
    ref_ev = [[(int(e["row"]), int(e["start"]), int(e["length"]), 0.0, float(e["gain"])) for e in row] for row in ev]
    assert ref_ev[0][1][1] < TILE < ref_ev[0][1][1] + ref_ev[0][1][2] and ref_ev[0][3][1] + ref_ev[0][3][2] == lens[0]
    fade = fade_ms * RATE // 1000
    assert fade == 0 or 2 * fade > 200
    want = synth_ref.render(clips, ref_rec, ref_ev, lens, got.wav.shape[1], fade=fade, noise=noise)
    assert np.abs(want).max() < 1.0 and got.wav.shape[1] >= max(lens)
    out = got.wav.cpu().numpy()
    for r, n in enumerate(lens):
        assert not out[r, n:].any(), "recording %d: samples past its length" % r
    print("max |error| %.3g" % np.abs(out - want).max())
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-6)
    # rows that start off a 16-byte boundary and hold no whole vectors: the scalar stores give the same bits
    from kws_amd import lib as L
    odd = got.wav.shape[1] + 3
    buf = torch.full((len(lens) * odd + 1,), 7.0, dtype=torch.float32, device="cuda")
    d_clips = torch.from_numpy(np.array(clips)).cuda()
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    L.check(L.get_lib().kws_synth_render(got.bank.handle(), d_clips.data_ptr(), L.WAV_I16 if dtype == "int16" else L.WAV_F32, 7, 200,
                                         got.rec.data_ptr(), got.plan.data_ptr(), got.plan.shape[1], d_len.data_ptr(), len(lens), max(lens), fade,
                                         buf.data_ptr() + 4, L.WAV_F32, odd, torch.cuda.current_stream().cuda_stream))
    assert float(buf[0]) == 7.0
    scalar = buf[1:].view(len(lens), odd).cpu().numpy()
    np.testing.assert_array_equal(scalar[:, :got.wav.shape[1]], out)
    assert not scalar[:, got.wav.shape[1]:].any()


def test_int16_output_is_the_rounded_float32_output(torch, store):
    """gain 40 on clips of amplitude 0.5 exceeds full scale: the int16 render saturates, bit for bit as rint-and-saturate of the float32
    render of the same arguments"""
    from kws_amd.synth import synthesize
    clips, valid, noise = store
    lens, plan, valid = _render_plan(valid, gain=40.0)
    args = dict(valid_len=valid, noise=noise, seconds=[n / RATE for n in lens], plan=plan, seed=2, **dict(KW, fade_ms=1, clip_cap=200))
    f = synthesize(clips, np.arange(7) % 5, out_dtype="float32", **args).wav.cpu().numpy()
    i = synthesize(clips, np.arange(7) % 5, out_dtype="int16", **args).wav
    assert i.dtype == torch.int16 and np.abs(f).max() > 1.0
    want = synth_ref.to_int16(f)
    assert want.max() == 32767 and want.min() == -32768
    np.testing.assert_array_equal(i.cpu().numpy(), want)


def test_end_to_end_sweep_of_a_synthesized_set(torch, tmp_path):
    """An untrained simple_cnn: synthesize at the default gaps, sweep at two operating points; the events are accepted by
    events_to_chunks; a second run and the saved files through Listener.sweep_wav give the same counts."""
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.stream import events_to_chunks
    from kws_amd.synth import synthesize
    from listen import Listener
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(8)
    clips = (0.3 * rng.standard_normal((10, 16000))).astype(np.float32)
    valid = rng.integers(6000, 16001, 10).astype(np.int32)
    labels = np.array([0, 1, 2, 3, 4, 1, 2, 3, 4, 0])
    noise = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (30000, 50000)]
    m = get_model("simple_cnn", 5)
    m.set_weights(init_weights(m.spec, seed=4))
    lis = Listener(model=m, classes_path=str(classes), chunk_size=1024)
    sens, levels = [0.05, 0.5], [1]                                     # this model fires at the first point and not at the second

    def run():
        s = synthesize(clips, labels, valid_len=valid, noise=noise, recordings=2, seconds=[20.0, 14.5], snr=[10.0], seed=5)
        return s, s.sweep(pr, m._device(), sens, levels, chunk_size=1024, class_names=NAMES, decoder=lis.threshold_decoder)

    def counts(res):
        return np.stack([t.cpu().numpy() for t in (res.fires, res.hits, res.false_alarms, res.duplicates, res.latency_chunks)], axis=-1)

    s, res = run()
    assert s.wav.dtype == torch.int16 and s.lengths == [320000, 232000]
    n_labelled = [len(e) for e in s.events]
    assert min(n_labelled) >= 3 and res.n_events == n_labelled and res.seconds == [20.0, 14.5]
    rec, _ = s.records()
    ref_rec, ref_ev = synth_ref.plan(clips, valid, s.lengths, 21, gap_lo=16000, gap_hi=48000, lead_in=16000, clip_cap=16000, seed=5,
                                     with_gains=False)
    assert [int(n) for n in rec["n_events"]] == [r[3] for r in ref_rec]
    assert s.events == synth_ref.labelled(ref_ev, ref_rec, labels)
    assert sum(n_labelled) < int(rec["n_events"].sum())                                        # the background's clips are in no event
    tol = s.tolerance_samples(1024, pr)
    assert 0 < tol <= pr.max_samples
    rows = events_to_chunks(s.events, s.lengths, 1024, tol)                                   # raises if two events' chunk ranges overlap
    assert [len(v) for v in rows] == n_labelled
    first = counts(res)
    print("fires per point", first[..., 0].sum(axis=0).tolist(), "hits", first[..., 1].sum(axis=0).tolist())
    assert first[..., 0].sum() > 0 and first[..., 1].sum() > 0, "no point fires inside an event: the comparisons below would be empty"
    s2, res2 = run()
    assert torch.equal(s2.wav, s.wav) and s2.events == s.events
    np.testing.assert_array_equal(counts(res2), first)
    paths, labels_path = s.save(str(tmp_path / "synth"), NAMES)
    from_files = lis.sweep_wav(paths, labels_path, sens, levels, tolerance_s=tol / float(pr.sample_rate))
    assert from_files.n_events == n_labelled
    np.testing.assert_array_equal(counts(from_files), first)


def test_listener_sweep_synth_from_a_dataset_folder(torch, tmp_path):
    """Plumbing of Listener.sweep_synth and `--sweep --synth_from`: a dataset folder and a noise folder give what synthesize and
    SynthSet.sweep give on the loaded arrays, and --save_dir collects the false alarms of the listener's point from the same scan."""
    from classifier.data import load_audio_samples, load_noise_bank
    from classifier.model import get_model
    from classifier.params import pr
    from common.data_utils import save_audio
    from kws_amd.init import init_weights
    from kws_amd.synth import synthesize
    from listen import Listener
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(12)
    for name in NAMES:
        (tmp_path / "data" / "sounds" / name).mkdir(parents=True)
        for i in range(2):
            save_audio(str(tmp_path / "data" / "sounds" / name / ("%d.wav" % i)), 0.3 * rng.standard_normal(int(rng.integers(6000, 16001))))
    (tmp_path / "noise").mkdir()
    save_audio(str(tmp_path / "noise" / "n.wav"), 0.1 * rng.standard_normal(40000))
    m = get_model("simple_cnn", 5)
    m.set_weights(init_weights(m.spec, seed=4))
    save_dir = tmp_path / "saved"
    lis = Listener(model=m, classes_path=str(classes), chunk_size=1024, sensitivity=0.05, trigger_level=1, save_dir=str(save_dir),
                   sweep=True, synth_from=str(tmp_path / "data"), noise_path=str(tmp_path / "noise"), synth_recordings=2, synth_seconds=12.0,
                   synth_snr="10", synth_seed=5, synth_save_dir=str(tmp_path / "synth"))
    res = lis.run_sweep()
    x, lengths, words = load_audio_samples(str(tmp_path / "data" / "sounds"), NAMES)
    direct = synthesize(x, [NAMES.index(w) for w in words], valid_len=lengths, noise=load_noise_bank(str(tmp_path / "noise")), recordings=2,
                        seconds=12.0, snr=[10.0], seed=5)
    assert torch.equal(lis.synth_set.wav, direct.wav) and lis.synth_set.events == direct.events and sum(len(e) for e in direct.events) > 0
    want = direct.sweep(pr, m._device(), [0.05], [1], chunk_size=1024, class_names=NAMES, decoder=lis.threshold_decoder)
    for a, b in ((res.fires, want.fires), (res.hits, want.hits), (res.false_alarms, want.false_alarms)):
        assert torch.equal(a, b)
    assert res.n_events == [len(e) for e in direct.events] and res.seconds == [12.0, 12.0]
    assert sorted(p.name for p in (tmp_path / "synth").iterdir()) == ["labels.txt", "synth_0.wav", "synth_1.wav"]
    n_false = int(res.false_alarms.sum())
    print("fires", int(res.fires.sum()), "false alarms", n_false)
    assert n_false > 0 and len(lis.collected_paths) == n_false == len(list(save_dir.rglob("*.wav")))
