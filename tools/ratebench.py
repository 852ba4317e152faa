"""Cost of per-slot sample rates: kws_amd.stream.StreamServer with S = 16 384 slots, chunk_size 1024, simple_cnn, every push naming
all slots (a fresh random order and chunk lengths, both drawn before the clock starts), in three configurations:
  native   every slot at the detector's rate: the path and launch count of tools/raggedbench.py's ragged_1 figure;
  mixed    a quarter of the slots each at 8, 16, 44.1 and 48 kHz, chunk lengths drawn in 1 .. the slot's own limit: one more launch,
           kws_rate_convert, in front of the ragged append;
  convert  kws_amd.rate.convert alone on --recordings recordings of 60 s at 44.1 kHz, with the bytes it moves and the FMAs it does
           computed from the shapes, over its time.
Every push (or convert call) sits between two HIP events; after a warm-up, the median and the spread are printed as ONE JSON line, as
tools/raggedbench.py does ("ms" is device time between the events, host gaps included; "host_ms" the host's wall time per call)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np
import torch

import kws_amd.lib as L
from classifier.params import pr
from kws_amd.init import init_weights
from kws_amd.model import DeviceModel, ModelSpec
from kws_amd.rate import bank_for, convert
from kws_amd.stream import StreamServer
from raggedbench import stats, timed

RATES = (8000, None, 44100, 48000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16384)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--model", default="simple_cnn")
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--only", default="native,mixed,convert")
    args = ap.parse_args()
    if args.pushes < 200:
        ap.error("--pushes must be at least 200")
    S, chunk = args.slots, 1024
    spec = ModelSpec(args.model, 36, pr.n_features, pr.n_mfcc)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, 0))
    names = ["background"] + ["w%d" % i for i in range(35)]
    rng = np.random.default_rng(0)
    res = {"tool": "ratebench", "slots": S, "chunk_size": chunk, "model": args.model, "device": torch.cuda.get_device_name(0),
           "build": {k: v for k, v in L.build_id().items() if k in ("kws_rate.hip", "kws_stream.hip", "kws_featurize.hip", "kws_featurize_v3.h")}}

    def server(rates):
        """-> a push function over pre-drawn (slots, lengths) for a server whose slot s arrives at rates[s % len(rates)]"""
        srv = StreamServer(pr, dm, S, chunk_size=chunk, class_names=names)
        for s in range(S):
            srv.open(sample_rate=rates[s % len(rates)])
        limit = srv.plan.max_chunk
        audio = (torch.randn((S, int(limit.max())), device="cuda") * 3000).to(torch.int16)
        n = args.warmup + args.pushes
        drawn = []
        for _ in range(n):
            slots = rng.permutation(S)
            drawn.append((slots, rng.integers(1, limit[slots] + 1)))

        def push(i):
            slots, lens = drawn[i % n]
            srv.push(slots, audio, lens)
        return srv, push

    only = args.only.split(",")
    if "native" in only:
        srv, push = server((None,))
        res["native"] = stats(*timed(args.warmup, args.pushes, push))
        res["native"]["launches_per_push"] = srv.launches / float(args.warmup + args.pushes)
    if "mixed" in only:
        srv, push = server(RATES)
        res["mixed"] = stats(*timed(args.warmup, args.pushes, push))
        res["mixed"]["launches_per_push"] = srv.launches / float(args.warmup + args.pushes)
        # where the device's share goes: ten more pushes under the library's per-launch timer, a pass of its own
        torch.cuda.synchronize()
        L.prof_enable(True)
        for i in range(10):
            push(i)
        rep = L.prof_report()
        L.prof_enable(False)
        res["mixed"]["kernel_ms_per_push"] = {k: round(v["total_ms"] / 10, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])}
    if "convert" in only:
        R, n_in = args.recordings, int(round(args.seconds * 44100))
        wav = (torch.randn((R, n_in), device="cuda") * 3000).to(torch.int16)
        bank = bank_for(44100, pr.sample_rate)
        n_out = bank.total(n_in)
        res["convert"] = stats(*timed(5, 30, lambda i: convert(wav, 44100, pr.sample_rate)))
        # the kernel's own begin -> end under the library's per-launch timer, in a pass of its own behind the timed one
        torch.cuda.synchronize()
        L.prof_enable(True)
        for _ in range(10):
            convert(wav, 44100, pr.sample_rate)
        rep = L.prof_report()
        L.prof_enable(False)
        ms = rep["rate_convert_kernel"]["total_ms"] / 10
        res["convert"]["kernel_ms"] = round(ms, 4)
        moved = R * 2 * (n_in + n_out) + bank.q * 2 * bank.taps * 4    # int16 in, int16 out, the bank once
        fmas = R * n_out * 2 * bank.taps
        res["convert"].update({"recordings": R, "samples_in": n_in, "samples_out": n_out, "taps": 2 * bank.taps, "bytes": moved, "fmas": fmas,
                               "GB_per_s": round(moved / ms * 1e-6, 1), "Gfma_per_s": round(fmas / ms * 1e-6, 1)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
