"""Cost of synthesizing labelled streaming test recordings (kws_amd.synth.synthesize: kws_synth_plan, kws_synth_render) at R = 64
recordings of 10 minutes from 1024 one-second int16 clips over a noise bank, int16 out.  In the same run, alternating within each round:
  plan     device time of kws_synth_plan (placement kernel + gain kernel), from events
  render   device time of kws_synth_render, from events, as a fraction of
  copy     a device-to-device copy of the same output bytes (read + write), and of the render's byte model at 8 TB/s
  host     the numpy restatement below (plan with gains, render) on --host_recordings of the recordings, wall time, scaled to R
The device's plan and samples are checked against the restatement on those recordings before anything is timed.  Prints one JSON
line; --out also writes it to a file.

    python tools/synthbench.py [--rounds 5] [--out profiles/synthbench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_GBS = 8000.0          # MI355X HBM3E peak
M32 = np.uint64(0xFFFFFFFF)


def np_hash(seed, step, index):
    """aug_hash (csrc/kws_wave_stage.h)"""
    index = np.asarray(index, np.uint64) & M32
    h = index ^ np.uint64((seed & 0xFFFFFFFF) ^ ((step * 0x27D4EB2F) & 0xFFFFFFFF))
    h = (h + np.uint64(((seed >> 32) + step) & 0xFFFFFFFF) * np.uint64(0x9E3779B9)) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def np_uniform(h, n):
    return ((h * np.asarray(n, np.uint64)) >> np.uint64(32)).astype(np.int64)


def host_plan(x, valid, noise, N, p, max_events, gap, lead_in, snr, bed, max_gain, seed):
    """one recording -> (segment, offset, bed_gain, rows, starts, lengths, gains) of the placed slots: include/kws.h in numpy"""
    h = np_hash(seed, p, np.arange(3))
    k = int(np_uniform(h[0], len(noise)))
    o = int(np_uniform(h[1], len(noise[k])))
    unit = np.float32(int(h[2]) >> 8) * np.float32(2.0 ** -24)
    g_bed = np.float32(np.float64(unit) * np.float64(np.float32(bed[1]) - np.float32(bed[0])) + np.float64(np.float32(bed[0])))
    j = np.arange(max_events, dtype=np.int64)
    row = np_uniform(np_hash(seed, p, 4 + 3 * j), len(x))
    gaps = gap[0] + np_uniform(np_hash(seed, p, 5 + 3 * j), gap[1] - gap[0] + 1)
    s_db = np.asarray(snr, np.float32)[np_uniform(np_hash(seed, p, 6 + 3 * j), len(snr))]
    ln = valid[row].astype(np.int64)
    end = lead_in + np.cumsum(ln + gaps)
    fits = end <= N
    n = max_events if fits.all() else int(np.argmin(fits))
    row, ln, start, s_db = row[:n], ln[:n], (end - ln)[:n], s_db[:n]
    seg = noise[k].astype(np.float64) ** 2
    pre = np.concatenate(([0.0], np.cumsum(seg)))
    gains = np.zeros(n, np.float32)
    for e in range(n):
        L = int(ln[e])
        if L == 0:
            continue
        p_v = float((x[row[e], :L].astype(np.float64) ** 2).sum()) / L
        a = (o + int(start[e])) % len(seg)
        n1 = min(L, len(seg) - a)
        rem = L - n1
        s = pre[a + n1] - pre[a] + (rem // len(seg)) * pre[-1] + pre[rem % len(seg)]
        p_n = float(g_bed) ** 2 * s / L
        gains[e] = min(np.float32(max_gain), np.float32(np.sqrt(10.0 ** (float(s_db[e]) / 10.0) * p_n / (p_v + float(np.finfo(np.float32).eps)))))
    return k, o, g_bed, row, start, ln, gains


def host_render(x, noise, N, plan, fade):
    """one recording -> int16 samples: the sample formula of include/kws.h in float32 numpy"""
    k, o, g_bed, row, start, ln, gains = plan
    n = noise[k]
    reps = -(-(o + N) // len(n))
    y = g_bed * np.tile(n, reps)[o:o + N]
    inv = np.float32(1.0) / np.float32(fade + 1)
    for e in range(len(row)):
        L = int(ln[e])
        u = np.arange(L)
        w = np.minimum(np.float32(1.0), np.minimum((u + 1).astype(np.float32) * inv, (L - u).astype(np.float32) * inv))
        a = int(start[e])
        y[a:a + L] = ((gains[e] * w).astype(np.float64) * x[row[e], :L] + y[a:a + L]).astype(np.float32)
    return np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="launches per timed window")
    ap.add_argument("--host_recordings", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from kws_amd.augment import NoiseBank
    from kws_amd.synth import synthesize
    rate, ms = 16000, 16000
    R, H = args.recordings, min(args.host_recordings, args.recordings)
    rng = np.random.default_rng(0)
    pcm = np.clip(rng.normal(0, 3000, (args.clips, ms)), -32768, 32767).astype(np.int16)
    valid = rng.integers(ms // 2, ms + 1, args.clips).astype(np.int32)
    labels = rng.integers(0, 12, args.clips)
    noise = [rng.normal(0, 0.1, n).astype(np.float32) for n in (60 * rate, 61 * rate + 7, 95 * rate + 1)]
    snr, bed, gap, fade, seed = [5.0, 10.0, 20.0], (0.05, 0.2), (rate, 3 * rate), 80, 1
    bank = NoiseBank(noise)
    s = synthesize(torch.from_numpy(pcm).cuda(), labels, valid_len=valid, noise=bank, recordings=R, seconds=args.seconds, snr=snr, bed_gain=bed,
                   seed=seed, sample_rate=rate, clip_cap=ms)
    rec, ev = s.records()
    N, max_events = s.lengths[0], ev.shape[1]

    # the device against the restatement, before anything is timed
    x = pcm.astype(np.float32) * np.float32(1.0 / 32768.0)
    host = lambda r: host_plan(x, valid, noise, N, r, max_events, gap, rate, snr, bed, 8.0, seed)      # noqa: E731
    plans = [host(r) for r in range(H)]
    got = s.wav[:H].cpu().numpy()
    worst = 0
    for r, p in enumerate(plans):
        n = int(rec["n_events"][r])
        assert (int(rec["segment"][r]), int(rec["offset"][r]), n) == (p[0], p[1], len(p[3])), "recording %d: plan differs from the host's" % r
        assert np.array_equal(ev["row"][r, :n], p[3]) and np.array_equal(ev["start"][r, :n], p[4]) and np.array_equal(ev["length"][r, :n], p[5])
        np.testing.assert_allclose(ev["gain"][r, :n], p[6], rtol=1e-5)
        dev_plan = (p[0], p[1], rec["bed_gain"][r], p[3], p[4], p[5], ev["gain"][r, :n])                   # the device's gains: the render alone
        worst = max(worst, int(np.abs(host_render(x, noise, N, dev_plan, fade).astype(np.int32) - got[r, :N]).max()))
    assert worst <= 1, "the device's samples differ from the host's by %d steps" % worst               # a rounding tie at most

    out_bytes = s.wav.numel() * s.wav.element_size()
    n_placed = int(rec["n_events"].sum())
    clip_samples = int(ev["length"].sum())
    # the render's byte model: every sample written once (2 B), the bed read once (4 B), the clips read once (2 B)
    model_bytes = out_bytes + 4 * R * N + 2 * clip_samples
    other = torch.empty_like(s.wav)
    variants = {"plan": s.replan, "render": s.rerender, "copy": lambda: other.copy_(s.wav)}
    times = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(device_ms(lambda: [fn() for _ in range(args.iters)]) / args.iters)
    t_host = []
    for _ in range(max(1, min(args.rounds, 2))):
        t0 = time.perf_counter()
        for r in range(H):
            host_render(x, noise, N, host(r), fade)
        t_host.append((time.perf_counter() - t0) * 1e3 * R / H)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"device": torch.cuda.get_device_name(0), "R": R, "seconds": args.seconds, "samples_per_recording": N, "clips": args.clips,
           "max_events": max_events, "events_placed": n_placed, "out_dtype": "int16", "out_bytes": out_bytes, "model_bytes": model_bytes,
           "plan_ms": {"median": round(med["plan"], 4), "rounds": [round(v, 4) for v in times["plan"]]},
           "render_ms": {"median": round(med["render"], 4), "rounds": [round(v, 4) for v in times["render"]]},
           "copy_ms": {"median": round(med["copy"], 4), "rounds": [round(v, 4) for v in times["copy"]]},
           "render_over_copy": round(med["render"] / med["copy"], 3),
           "render_gbs_model": round(model_bytes / med["render"] / 1e6, 1),
           "render_share_of_8tbs": round(model_bytes / (HBM_GBS * 1e6) / med["render"], 4),
           "copy_gbs": round(2 * out_bytes / med["copy"] / 1e6, 1),
           "host_ms_scaled_to_R": {"median": round(statistics.median(t_host), 1), "rounds": [round(v, 1) for v in t_host], "recordings_run": H},
           "host_over_device": round(statistics.median(t_host) / (med["plan"] + med["render"]), 1),
           "max_abs_int16_diff_vs_host": worst}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
