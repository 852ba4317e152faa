"""Cost of a ragged push: kws_amd.stream.StreamServer with S = 16 384 slots, chunk_size 1024, simple_cnn, at the active fractions
1.0, 0.5, 0.1 and 0.01 -- every push names a fresh random subset of the slots with each chunk's length drawn in 1..1024 (both
drawn before the clock starts) -- and StreamBatch.push at the same S in the same run.  Every push sits between two HIP events; after a warm-up, the median and the
spread over --pushes pushes are printed as ONE JSON line ("ms" is device time between the events, which includes the gaps the host
leaves while it builds the next launch; "host_ms" is the host's wall time per push over the same loop, device drained at its end).

--prof runs no timing at all: it replays a few all-active pushes of both classes under the library's per-kernel timing
(kws_prof_enable) and prints where the time goes, a run of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np
import torch

import kws_amd.lib as L
from classifier.params import pr
from kws_amd.init import init_weights
from kws_amd.model import DeviceModel, ModelSpec
from kws_amd.stream import StreamBatch, StreamServer

FRACTIONS = (1.0, 0.5, 0.1, 0.01)


def timed(n_warm, n, push):
    """-> (device ms per push as a list, host ms per push)"""
    for i in range(n_warm):
        push(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    t0 = time.perf_counter()
    for i, (a, b) in enumerate(ev):
        a.record()
        push(n_warm + i)
        b.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / n * 1e3
    return [a.elapsed_time(b) for a, b in ev], host


def stats(ms, host):
    v = np.sort(np.asarray(ms))
    return {"ms": round(float(np.median(v)), 4), "p10": round(float(v[len(v) // 10]), 4), "p90": round(float(v[(9 * len(v)) // 10]), 4),
            "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4), "host_ms": round(host, 4), "pushes": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16384)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--model", default="simple_cnn")
    ap.add_argument("--prof", action="store_true", help="per-kernel times of all-active pushes instead of the timing")
    args = ap.parse_args()
    if args.pushes < 200 and not args.prof:
        ap.error("--pushes must be at least 200")
    S, chunk = args.slots, 1024
    spec = ModelSpec(args.model, 36, pr.n_features, pr.n_mfcc)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, 0))
    names = ["background"] + ["w%d" % i for i in range(35)]
    srv = StreamServer(pr, dm, S, chunk_size=chunk, class_names=names)
    sb = StreamBatch(pr, dm, S, chunk_size=chunk, class_names=names)
    for _ in range(S):
        srv.open()
    audio = (torch.randn((S, chunk), device="cuda") * 3000).to(torch.int16)
    rng = np.random.default_rng(0)

    def ragged(fraction, n):
        """a push function over n pre-drawn (slots, lengths): the draw is the caller's work, not the push's"""
        A = max(1, int(round(S * fraction)))
        drawn = [(rng.choice(S, A, replace=False) if A < S else rng.permutation(S), rng.integers(1, chunk + 1, A)) for _ in range(n)]

        def push(i):
            slots, lens = drawn[i % n]
            srv.push(slots, audio[:A], lens)
        return push

    if args.prof:
        out = {}
        for name, push in (("ragged_1.0", ragged(1.0, args.warmup + 10)), ("stream_batch", lambda i: sb.push(audio))):
            for i in range(args.warmup):
                push(i)
            torch.cuda.synchronize()
            L.prof_enable(True)
            for i in range(10):
                push(i)
            rep = L.prof_report()
            L.prof_enable(False)
            out[name] = {k: round(v["total_ms"] / 10, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])}
        print(json.dumps({"tool": "raggedbench", "mode": "prof", "slots": S, "model": args.model, "kernel_ms_per_push": out}))
        return
    res = {"tool": "raggedbench", "slots": S, "chunk_size": chunk, "model": args.model, "device": torch.cuda.get_device_name(0),
           "build": {k: v for k, v in L.build_id().items() if k in ("kws_stream.hip", "kws_featurize.hip", "kws_featurize_v3.h")}}
    res["stream_batch"] = stats(*timed(args.warmup, args.pushes, lambda i: sb.push(audio)))
    for f in FRACTIONS:
        res["ragged_%g" % f] = stats(*timed(args.warmup, args.pushes, ragged(f, args.warmup + args.pushes)))
    res["stream_batch_again"] = stats(*timed(args.warmup, args.pushes, lambda i: sb.push(audio)))        # the run's drift
    print(json.dumps(res))


if __name__ == "__main__":
    main()
