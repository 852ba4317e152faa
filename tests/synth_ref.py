"""numpy restatement of the streaming-recording synthesis (include/kws.h: kws_synth_plan, kws_synth_render; csrc/kws_synth.hip), built on
tests/aug_ref.py's draws: the draws and starts in integers, the gains in float64, the render in float32 steps.  Shared by
tests/test_synth_host.py (its own invariants) and tests/test_synth_gpu.py (the kernels against it)."""
import numpy as np

from aug_ref import np_hash, np_uniform, np_unit

F32_EPS = float(np.finfo(np.float32).eps)
EMPTY = (-1, 0, 0, 0.0, 0.0)


def to_f32(clips):
    """aug_to_f32: int16 scaled by 1/32768"""
    clips = np.asarray(clips)
    return clips.astype(np.float32) * np.float32(1.0 / 32768.0) if clips.dtype == np.int16 else clips.astype(np.float32)


def clip_lengths(valid_len, rows, stride, clip_cap):
    v = np.full(rows, stride, np.int64) if valid_len is None else np.asarray(valid_len, np.int64)
    return np.minimum(np.clip(v, 0, stride), clip_cap)


def circular_power(seg, a, n):
    """sum of seg[(a + i) mod len(seg)]^2 over i < n in float64"""
    sq = seg.astype(np.float64) ** 2
    idx = (a + np.arange(n, dtype=np.int64)) % len(seg)
    return float(sq[idx].sum())


def plan(clips, valid_len, lengths, max_events, gap_lo, gap_hi, lead_in, clip_cap, snr_db=(), bed_gain=(0.0, 0.0), max_gain=8.0, seed=0,
         pick=None, noise=None, position_base=0, with_gains=True):
    """-> (rec, events): rec[r] = (segment, offset, bed_gain float32, n_events); events[r] = max_events tuples (row, start, length,
    snr_db, gain), EMPTY at or past n_events.  clips (rows, stride) float32 / int16, noise: list of float32 segments or None."""
    clips = np.asarray(clips)
    rows, stride = clips.shape
    x = to_f32(clips) if with_gains else None
    lens = clip_lengths(valid_len, rows, stride, clip_cap)
    M = rows if pick is None else len(pick)
    snr_db = [np.float32(s) for s in snr_db]
    lo, hi = np.float32(bed_gain[0]), np.float32(bed_gain[1])
    rec, events = [], []
    for r, N in enumerate(lengths):
        p = (position_base + r) & 0xFFFFFFFF
        seg, off, bed = -1, 0, np.float32(0)
        if noise is not None:
            h = np_hash(seed, p, np.arange(3))
            seg = int(np_uniform(h[0], len(noise)))
            off = int(np_uniform(h[1], len(noise[seg])))
            bed = np.float32(np.float64(np_unit(h[2:3])[0]) * np.float64(np.float32(hi - lo)) + np.float64(lo))    # fmaf: one rounding
        j = np.arange(max_events, dtype=np.int64)
        sel = np_uniform(np_hash(seed, p, 4 + 3 * j), M)
        row = sel if pick is None else np.asarray(pick, np.int64)[sel]
        gap = gap_lo + np_uniform(np_hash(seed, p, 5 + 3 * j), gap_hi - gap_lo + 1)
        snr = np.zeros(max_events, np.float32)
        if snr_db:
            snr = np.asarray(snr_db, np.float32)[np_uniform(np_hash(seed, p, 6 + 3 * j), len(snr_db))]
        ln = lens[row]
        end = lead_in + np.cumsum(ln + gap)
        start = end - ln
        fits = end <= N
        n_ev = max_events if fits.all() else int(np.argmin(fits))
        evs = []
        for e in range(max_events):
            if e >= n_ev:
                evs.append(EMPTY)
                continue
            L = int(ln[e])
            g = 1.0 if L > 0 else 0.0
            if with_gains and L > 0 and snr_db and noise is not None:
                p_v = float((x[row[e], :L].astype(np.float64) ** 2).sum()) / L
                p_n = float(bed) ** 2 * circular_power(noise[seg], off + int(start[e]), L) / L
                g = min(float(np.float32(max_gain)), float(np.float32(np.sqrt(10.0 ** (float(snr[e]) / 10.0) * p_n / (p_v + F32_EPS)))))
            evs.append((int(row[e]), int(start[e]), L, float(snr[e]), g))
        rec.append((seg, off, bed, n_ev))
        events.append(evs)
    return rec, events


def render(clips, rec, events, lengths, out_stride, fade=0, noise=None):
    """-> (R, out_stride) float32: the sample formula of include/kws.h in float32 steps (each product rounded, one fused
    multiply-add emulated in float64: a float32 product is exact there, and the sum is rounded to float32 once more -- a double
    rounding that can differ from the fused result by one float32 ulp in rare cases, far below the tests' 1e-6)."""
    x = to_f32(clips)
    inv_fade = np.float32(1.0) / np.float32(fade + 1)
    out = np.zeros((len(lengths), out_stride), np.float32)
    for r, N in enumerate(lengths):
        seg, off, bed, n_ev = rec[r]
        y = np.zeros(N, np.float32)
        if noise is not None and seg >= 0 and N > 0:
            n = noise[seg].astype(np.float32)
            y = np.float32(bed) * n[(off + np.arange(N, dtype=np.int64)) % len(n)]
        for row, start, L, _, gain in events[r][:n_ev]:
            if L <= 0:
                continue
            u = np.arange(L, dtype=np.int64)
            w = np.minimum(np.float32(1.0), np.minimum((u + 1).astype(np.float32) * inv_fade, (L - u).astype(np.float32) * inv_fade))
            gw = np.float32(gain) * w
            y[start:start + L] = (gw.astype(np.float64) * x[row, :L].astype(np.float64) + y[start:start + L].astype(np.float64)).astype(np.float32)
        out[r, :N] = y
    return out


def to_int16(x):
    """rint(x * 32768) saturated to [-32768, 32767]"""
    return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def labelled(events, rec, labels, background_index=0):
    """per recording the (class_index, start, end) of the placed, non-empty, non-background clips"""
    out = []
    for r, evs in enumerate(events):
        out.append([(int(labels[row]), start, start + L) for row, start, L, _, _ in evs[:rec[r][3]] if L > 0 and int(labels[row]) != background_index])
    return out
