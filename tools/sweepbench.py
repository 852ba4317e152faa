"""Operating-point sweep against the route it replaces, on synthetic probabilities (a sweep needs no model): R recordings of
60 s at chunk 1024 and P = 17 x 5 operating points.

  repeated  P calls of kws_stream_scan_postprocess on the same (R, K, C) probabilities, one per point, each from a fresh
            detector state (decode + trigger walk every time: the entry point offers no walk alone);
  sweep     one kws_stream_sweep launch on the index / score the first of those calls wrote, without and with labelled events.

Device times from CUDA events around the enqueued calls, alternating, medians over --rounds; the fires of the sweep are checked
against the repeated calls' fired flags before anything is timed.

    python tools/sweepbench.py [--rounds 5] [--out profiles/sweepbench.json]

Put the same command under rocprofv3 --kernel-trace --stats (with a smaller --rounds) for the per-kernel record."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import numpy as np
import torch

from classifier.params import pr
from kws_amd import lib as L
from kws_amd.stream import ThresholdDecoder, events_to_chunks


def synthetic_probs(R, K, C, seed=0):
    """(R, K, C) float32 probabilities: noise plus runs of 8 chunks of one class with a random margin, so that detections happen
    at some operating points and not at others"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn((R, K, C), device="cuda", generator=g)
    runs = -(-K // 8)
    cls = torch.randint(0, C, (R, runs), device="cuda", generator=g).repeat_interleave(8, dim=1)[:, :K]
    gain = (14.0 * torch.rand((R, runs), device="cuda", generator=g)).repeat_interleave(8, dim=1)[:, :K]
    logits.scatter_add_(2, cls.unsqueeze(-1), gain.unsqueeze(-1))
    return torch.softmax(logits, dim=-1).contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--chunk_size", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sweepbench needs a HIP device"
    R, C, chunk = args.recordings, args.classes, args.chunk_size
    N = args.seconds * pr.sample_rate
    K = -(-N // chunk)
    sens = [0.1 + 0.8 * i / 16 for i in range(17)]
    levels = [1, 2, 3, 4, 5]
    points = [(s, l) for s in sens for l in levels]
    P = len(points)
    lib = L.get_lib()
    st = torch.cuda.current_stream().cuda_stream
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    probs = synthetic_probs(R, K, C)
    d_chunks = torch.full((R,), K, dtype=torch.int32, device="cuda")
    index = torch.empty((R, K), dtype=torch.int32, device="cuda")
    score = torch.empty((R, K), dtype=torch.float64, device="cuda")
    fired = torch.empty((R, K), dtype=torch.int32, device="cuda")
    states = torch.empty((P, R, 2), dtype=torch.int32, device="cuda")
    d_sens = torch.tensor([p[0] for p in points], dtype=torch.float64, device="cuda")
    d_level = torch.tensor([p[1] for p in points], dtype=torch.int32, device="cuda")
    counts = torch.empty((R, P, 5), dtype=torch.int32, device="cuda")
    # labels: one event of a random class every 6 s, 0.5 s long, the default tolerance (the model's buffer)
    rng = np.random.default_rng(0)
    events = [[(int(rng.integers(1, C)), t * pr.sample_rate, t * pr.sample_rate + pr.sample_rate // 2) for t in range(2, args.seconds - 1, 6)]
              for _ in range(R)]
    rows = events_to_chunks(events, [N] * R, chunk, pr.max_samples, 0, C)
    off = np.concatenate(([0], np.cumsum([len(v) for v in rows]))).astype(np.int32)
    flat = np.array([e for v in rows for e in v], dtype=np.int32).reshape(-1, 3)
    ev = [torch.from_numpy(off).cuda()] + [torch.from_numpy(np.ascontiguousarray(flat[:, i])).cuda() for i in range(3)]

    def one_point(i):
        s, l = points[i]
        L.check(lib.kws_stream_scan_postprocess(dec.handle, probs.data_ptr(), R, K, C, d_chunks.data_ptr(), 0, 0, s, l, chunk,
                                                states[i].data_ptr(), index.data_ptr(), score.data_ptr(), fired.data_ptr(), K, st))

    def reset_states():
        states[..., 0] = 0
        states[..., 1] = -1

    def repeated():
        for i in range(P):
            one_point(i)

    def run_sweep(labelled):
        e = [t.data_ptr() for t in ev] if labelled else [0, 0, 0, 0]
        L.check(lib.kws_stream_sweep(index.data_ptr(), score.data_ptr(), R, K, d_chunks.data_ptr(), 0, chunk, d_sens.data_ptr(),
                                     d_level.data_ptr(), P, e[0], e[1], e[2], e[3], counts.data_ptr(), st))

    # correctness first (doubles as the warm-up): per point, the repeated route's fired flags summed are the sweep's fires
    reset_states()
    want = torch.empty((R, P), dtype=torch.int64, device="cuda")
    for i in range(P):
        one_point(i)
        want[:, i] = fired.sum(dim=1)
    run_sweep(False)
    assert torch.equal(counts[..., 0].long(), want), "the sweep's fires differ from the repeated route's"
    run_sweep(True)
    assert torch.equal(counts[..., 0].long(), want)
    labelled_counts = counts.sum(dim=(0, 1)).tolist()
    fires_per_point = want.sum(dim=0)
    t_rep, t_sweep, t_lab = [], [], []
    for _ in range(args.rounds):                                     # alternating
        reset_states()
        torch.cuda.synchronize()
        t_rep.append(timed(repeated))
        t_sweep.append(timed(lambda: run_sweep(False)))
        t_lab.append(timed(lambda: run_sweep(True)))
    rec = {"device": torch.cuda.get_device_name(0), "R": R, "K": K, "P": P, "C": C, "chunk_size": chunk, "events": int(flat.shape[0]),
           "rounds": args.rounds, "repeated_postprocess_ms": t_rep, "sweep_ms": t_sweep, "sweep_labelled_ms": t_lab,
           "repeated_postprocess_median_ms": statistics.median(t_rep), "sweep_median_ms": statistics.median(t_sweep),
           "sweep_labelled_median_ms": statistics.median(t_lab),
           "points_that_fire": int((fires_per_point > 0).sum()), "fires_min_max": [int(fires_per_point.min()), int(fires_per_point.max())],
           "labelled_totals": dict(zip(("fires", "hits", "false_alarms", "duplicates", "latency_chunks"), labelled_counts))}
    rec["repeated_over_sweep"] = rec["repeated_postprocess_median_ms"] / rec["sweep_labelled_median_ms"]
    print("R %d K %d P %d: %d x scan_postprocess %.3f ms | sweep %.3f ms, labelled %.3f ms | ratio %.1f x | %d of %d points fire"
          % (R, K, P, P, rec["repeated_postprocess_median_ms"], rec["sweep_median_ms"], rec["sweep_labelled_median_ms"],
             rec["repeated_over_sweep"], rec["points_that_fire"], P), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
