"""Query-by-example search in figures (kws_dtw, csrc/kws_dtw.hip):

  one hour      one recording of one hour (112499 rows of 20 MFCCs) against 1 and against 16 templates of 40 rows;
  many minutes  256 recordings of one minute (1874 rows each) against 16 templates of 40 rows.

Each workload runs with tile_frames = 0 (the library cuts the frames into jobs) and again with the tile forced to the whole recording,
which is one wave per (recording, template) pair.  The second run of "one hour" against one template is ONE wave alone on the chip: its
time over its steps is the latency of one step of the wave, with nothing to hide it behind.

The tool reports the time of the dtw_kernel launch alone (the library's per-launch timing), the time of the whole kws_amd.qbe.match_rows
call between device events (which adds the two kws_rows_normalize launches of the cosine metric), the DP cells per second (template
rows x frames x templates x recordings over the kernel time) and the multiple of real time (seconds of audio over the kernel time).
Before anything is timed the tiled and the untiled results are compared bit for bit.  The tool reports, it asserts no ratio.

    python tools/dtwbench.py [--rounds 5] [--out profiles/dtwbench.json]

Every figure is the median of --rounds repetitions after two warm-up runs of the same work.  The last line printed is the record as
one JSON line."""
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

from kws_amd import lib as _l
from kws_amd import qbe

RATE, WINDOW, HOP, D, ROWS = 16000, 1024, 512, 20, 40
HOUR, MINUTE = 3600, 60


def frames(seconds):
    return (seconds * RATE - WINDOW) // HOP + 1


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(fn):
    _l.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    rep = _l.prof_report()
    _l.prof_enable(False)
    return rep["dtw_kernel"]["total_ms"]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def one_run(t, rows, n, tile, rounds, seconds):
    R, F = int(rows.shape[0]), int(rows.shape[1])
    run = lambda: qbe.match_rows(t, rows, n, "cosine", tile_frames=tile)
    for _ in range(2):
        out = run()
    t_k, t_c = [], []
    for _ in range(rounds):
        t_k.append(kernel_ms(run))
        t_c.append(event_ms(run))
    k_ms = statistics.median(t_k)
    cells = float(ROWS) * F * len(t) * R
    rec = {"tile_frames": tile, "kernel_ms": med(t_k), "call_ms": med(t_c), "cells_per_second": cells / (k_ms * 1e-3),
           "times_real_time": R * seconds / (k_ms * 1e-3)}
    return rec, out


def workload(name, R, seconds, Q, rounds, rng):
    F = frames(seconds)
    rows = torch.from_numpy(rng.standard_normal((R, F, D)).astype(np.float32)).cuda()
    n = np.full((R,), F, np.int32)
    t = qbe.Templates.from_rows(torch.from_numpy(rng.standard_normal((Q, ROWS, D)).astype(np.float32)).cuda(), np.full((Q,), ROWS, np.int32),
                                ["w%d" % (q % 4) for q in range(Q)])
    whole = min(max(F, 32), 2 ** 20)
    tiled, a = one_run(t, rows, n, 0, rounds, seconds)
    untiled, b = one_run(t, rows, n, whole, rounds, seconds)
    same = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
    rec = {"workload": name, "recordings": R, "seconds_each": seconds, "frames_each": F, "templates": Q, "template_rows": ROWS, "D": D,
           "tiled": tiled, "untiled": untiled, "untiled_over_tiled": untiled["kernel_ms"]["median"] / tiled["kernel_ms"]["median"],
           "tiled_and_untiled_bits_equal": same}
    if R == 1 and Q == 1:
        rec["one_wave_ns_per_step"] = untiled["kernel_ms"]["median"] * 1e6 / F
    print("%-12s R %3d Q %2d: tiled %9.3f ms (%.3g cells/s, %.0f x real time), one wave per pair %9.3f ms: %.1f x; same bits: %s"
          % (name, R, Q, tiled["kernel_ms"]["median"], tiled["cells_per_second"], tiled["times_real_time"], untiled["kernel_ms"]["median"],
             rec["untiled_over_tiled"], same), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "conditions": "two warm-up runs of the same work first, then the median of `rounds` repetitions (min and max kept); kernel_ms is "
                            "the library's per-launch timing of dtw_kernel, call_ms device events around the whole match_rows call (cosine: "
                            "two kws_rows_normalize launches more); random rows; untiled = tile_frames forced to the whole recording",
              "build_id": {k: _l.build_id().get(k) for k in ("kws_dtw.hip",)}}
    record["workloads"] = [workload("one hour", 1, HOUR, 1, args.rounds, rng), workload("one hour", 1, HOUR, 16, args.rounds, rng),
                           workload("many minutes", 256, MINUTE, 16, args.rounds, rng)]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
