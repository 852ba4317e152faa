"""Harvest of a scan (kws_amd.stream.collect / peaks / Detections.clips) against a host restatement that walks the same scan
output file by file, on synthetic probabilities and random PCM (mining needs no model): R recordings of 60 s at chunk 1024.

  device  collect (a counting launch, its read-back, the storing launch) + peaks + the clips of both, on the index / score one
          kws_stream_scan_postprocess call wrote and a packed int16 buffer that is already on the device;
  host    the same index / score copied to the host once (not timed), then per recording: TriggerDetector.update chunk by chunk
          with the event bookkeeping, the greedy peak pick with numpy, and every clip cut from the host PCM and scaled.

Wall-clock times around synchronised calls (collect reads its counts back, so events alone would not cover it), alternating,
medians over --rounds; the device's detections, peaks and clips are checked against the host's before anything is timed.

    python tools/minebench.py [--rounds 5] [--out profiles/minebench.json]

Put the same command under rocprofv3 --kernel-trace --stats (with a smaller --rounds) for the per-kernel record."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import numpy as np
import torch

from classifier.params import pr
from kws_amd import lib as L
from kws_amd.stream import ThresholdDecoder, collect, events_to_chunks, peaks
from tools.sweepbench import synthetic_probs


def host_detections(index, score, sens, level, chunk, events):
    """one recording -> [(chunk, class, kind, event)]: listen.py:538-559 chunk by chunk, kinds by the sweep's rule"""
    act, rec, out = 0, -1, []
    e, found = 0, False
    refractory = -(8 * 2048) // chunk
    for k in range(len(index)):
        idx, sc = int(index[k]), float(score[k])
        if idx != 0 and idx == rec and sc > sens:
            act += 1
            if act > level:
                act = refractory
                while e < len(events) and events[e][2] < k:
                    e += 1
                    found = False
                if e < len(events) and events[e][1] <= k and events[e][0] == idx:
                    out.append((k, idx, 2 if found else 1, e))
                    found = True
                else:
                    out.append((k, idx, 3, -1))
                continue
        elif act < 0:
            act += 1
        elif act > 0:
            act -= 1
        rec = idx
    return out


def host_peaks(index, score, min_score, min_gap, K, events):
    """one recording -> [(chunk, class)]: numpy masks, np.argmax returns the first maximum (the lowest chunk among ties)"""
    ok = (index != 0) & (score > min_score)
    for _, lo, hi in events:
        ok[lo:hi + 1] = False
    s = np.where(ok, score, -np.inf)
    out = []
    while len(out) < K:
        k = int(np.argmax(s)) if s.size else 0
        if s.size == 0 or s[k] == -np.inf:
            break
        out.append((k, int(index[k])))
        s[max(0, k - min_gap + 1):k + min_gap] = -np.inf
    return out


def host_clips(pcm, chunks, chunk, B):
    out = np.zeros((len(chunks), B), np.float32)
    for i, k in enumerate(chunks):
        end = min((k + 1) * chunk, pcm.size)
        cut = pcm[max(0, end - B):end]
        out[i, B - cut.size:] = cut.astype(np.float32) / 32768.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=256)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--chunk_size", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=36)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "minebench needs a HIP device"
    R, C, chunk, K = args.recordings, args.classes, args.chunk_size, args.k
    N = args.seconds * pr.sample_rate
    T = -(-N // chunk)
    B = pr.buffer_samples
    gap = -(-B // chunk)
    sens, level = 0.5, 3
    lib = L.get_lib()
    st = torch.cuda.current_stream().cuda_stream
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    probs = synthetic_probs(R, T, C)
    n_chunks = [T] * R
    d_chunks = torch.full((R,), T, dtype=torch.int32, device="cuda")
    index = torch.empty((R, T), dtype=torch.int32, device="cuda")
    score = torch.empty((R, T), dtype=torch.float64, device="cuda")
    fired = torch.empty((R, T), dtype=torch.int32, device="cuda")
    state = torch.zeros((R, 2), dtype=torch.int32, device="cuda")
    state[:, 1] = -1
    L.check(lib.kws_stream_scan_postprocess(dec.handle, probs.data_ptr(), R, T, C, d_chunks.data_ptr(), 0, 0, sens, level, chunk,
                                            state.data_ptr(), index.data_ptr(), score.data_ptr(), fired.data_ptr(), T, st))
    g = torch.Generator(device="cuda").manual_seed(1)
    wav = torch.randint(-32768, 32768, (R, N), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    # labels: one event of a random class every 6 s, 0.5 s long, the default tolerance (the model's buffer)
    rng = np.random.default_rng(0)
    events = [[(int(rng.integers(1, C)), t * pr.sample_rate, t * pr.sample_rate + pr.sample_rate // 2) for t in range(2, args.seconds - 1, 6)]
              for _ in range(R)]
    rows = events_to_chunks(events, [N] * R, chunk, pr.max_samples, 0, C)
    scan = (index, score, n_chunks)
    kw = dict(events=events, lengths=[N] * R, pr=pr)

    def device():
        det = collect(scan, chunk, sens, level, **kw)
        pk = peaks(scan, chunk, k=K, min_score=0.0, **kw)
        return det, pk, det.clips(wav, lengths=[N] * R, pr=pr), pk.clips(wav, lengths=[N] * R, pr=pr)

    h_index, h_score, h_wav = index.cpu().numpy(), score.cpu().numpy(), wav.cpu().numpy()

    def host():
        dets, pks, clips = [], [], []
        for r in range(R):
            d = host_detections(h_index[r], h_score[r], sens, level, chunk, rows[r])
            p = host_peaks(h_index[r], h_score[r], 0.0, gap, K, rows[r])
            dets.append(d)
            pks.append(p)
            clips.append(host_clips(h_wav[r], [v[0] for v in d] + [v[0] for v in p], chunk, B))
        return dets, pks, clips

    # correctness first (doubles as the warm-up)
    det, pk, det_clips, pk_clips = device()
    dets, pks, clips = host()
    assert list(zip(det.recording.tolist(), det.chunk.tolist(), det.cls.tolist(), det.kind.tolist(), det.event.tolist())) == \
        [(r,) + v for r, d in enumerate(dets) for v in d], "the device's detections differ from the host's"
    assert list(zip(pk.recording.tolist(), pk.chunk.tolist(), pk.cls.tolist())) == [(r,) + v for r, p in enumerate(pks) for v in p], \
        "the device's peaks differ from the host's"
    h_det_clips = np.concatenate([c[:len(d)] for c, d in zip(clips, dets)])
    h_pk_clips = np.concatenate([c[len(d):] for c, d in zip(clips, dets)])
    assert np.array_equal(det_clips.cpu().numpy(), h_det_clips) and np.array_equal(pk_clips.cpu().numpy(), h_pk_clips)
    kinds = torch.bincount(det.kind.long(), minlength=4).tolist()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def kernels_only():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_det = torch.empty(R, dtype=torch.int32, device="cuda")
        cap = max(det.n + [1])
        out = torch.empty((R, cap, 4), dtype=torch.int32, device="cuda")
        out_score = torch.empty((R, cap), dtype=torch.float64, device="cuda")
        n_pk = torch.empty(R, dtype=torch.int32, device="cuda")
        pk_out = torch.empty((R, K, 2), dtype=torch.int32, device="cuda")
        pk_score = torch.empty((R, K), dtype=torch.float64, device="cuda")
        from kws_amd.stream import _event_tensors
        ev = [t.data_ptr() for t in _event_tensors(torch, rows, "cuda")]
        torch.cuda.synchronize()
        a.record()
        L.check(lib.kws_stream_collect(index.data_ptr(), score.data_ptr(), R, T, d_chunks.data_ptr(), 0, chunk, sens, level, ev[0], ev[1],
                                       ev[2], ev[3], cap, n_det.data_ptr(), out.data_ptr(), out_score.data_ptr(), st))
        b.record()
        b.synchronize()
        t_collect = a.elapsed_time(b)
        a.record()
        L.check(lib.kws_stream_peaks(index.data_ptr(), score.data_ptr(), R, T, d_chunks.data_ptr(), 0, 0.0, gap, ev[0], ev[2], ev[3], K,
                                     n_pk.data_ptr(), pk_out.data_ptr(), pk_score.data_ptr(), st))
        b.record()
        b.synchronize()
        return t_collect, a.elapsed_time(b)

    t_dev, t_host, t_ck, t_pk = [], [], [], []
    for _ in range(args.rounds):                                     # alternating
        t_dev.append(wall(device))
        t_host.append(wall(host))
        c, p = kernels_only()
        t_ck.append(c)
        t_pk.append(p)
    rec = {"device": torch.cuda.get_device_name(0), "R": R, "chunks_per_recording": T, "C": C, "chunk_size": chunk, "k": K, "min_gap": gap,
           "sensitivity": sens, "trigger_level": level, "events": sum(len(v) for v in rows), "rounds": args.rounds,
           "detections": len(det), "kinds": dict(zip(("unlabelled", "hits", "duplicates", "false_alarms"), kinds)), "peaks": len(pk),
           "clip_samples": B, "device_wall_ms": t_dev, "host_wall_ms": t_host, "collect_kernel_ms": t_ck, "peaks_kernel_ms": t_pk,
           "device_wall_median_ms": statistics.median(t_dev), "host_wall_median_ms": statistics.median(t_host),
           "collect_kernel_median_ms": statistics.median(t_ck), "peaks_kernel_median_ms": statistics.median(t_pk)}
    rec["host_over_device"] = rec["host_wall_median_ms"] / rec["device_wall_median_ms"]
    print("R %d T %d: %d detections %s, %d peaks | device %.3f ms (collect kernel %.3f, peaks kernel %.3f) | host %.1f ms | ratio %.1f x"
          % (R, T, len(det), kinds, len(pk), rec["device_wall_median_ms"], rec["collect_kernel_median_ms"], rec["peaks_kernel_median_ms"],
             rec["host_wall_median_ms"], rec["host_over_device"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
