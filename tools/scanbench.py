"""Offline scan against the chunk loop on recorded audio: Listener.run_wav (one 1024-sample chunk per step, S = 1) and
Listener.scan_wav (kws_amd.stream.scan) over the same synthetic wav files, alternating, medians of wall-clock time around
a device synchronisation; plus the scan's per-stage device times (rows / gather / forward / scan) from CUDA events.

    python tools/scanbench.py [--rounds 3] [--out profiles/scan_bench.json] [--only 60min] [--scan_only]

--scan_only runs nothing but warmed-up scans (the process to put under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import numpy as np
import torch

from classifier.model import get_model
from classifier.params import pr
from kws_amd.featurizer import Featurizer
from kws_amd.init import init_weights
from kws_amd.quant import calibrate, quantized_class
from kws_amd.stream import scan
from listen import Listener

WORKLOADS = {"10min": (1, 600), "60min": (1, 3600), "64x1min": (64, 60)}      # files, seconds each
MODELS = [("simple_cnn", False), ("simple_cnn_lite", False), ("simple_cnn", True)]
NAMES = ["background"] + ["w%d" % i for i in range(35)]


def write_wavs(folder, tag, files, seconds):
    rng = np.random.default_rng(len(tag) + files)
    paths = []
    for i in range(files):
        pcm = np.clip(rng.normal(0, 3000, seconds * pr.sample_rate), -32768, 32767).astype(np.int16)
        paths.append(os.path.join(folder, "%s_%02d.wav" % (tag, i)))
        with wave.open(paths[-1], "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(pr.sample_rate)
            wf.writeframes(pcm.tobytes())
    return paths


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--only", type=str, default=None)
    ap.add_argument("--scan_only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="scanbench_")
    with open(os.path.join(tmp, "classes.txt"), "w") as f:
        f.write("\n".join(NAMES) + "\n")
    records = []
    for tag, (files, seconds) in WORKLOADS.items():
        if args.only and tag != args.only:
            continue
        paths = write_wavs(tmp, tag, files, seconds)
        audio_s = files * seconds
        for model_type, int8 in MODELS:
            m = get_model(model_type, len(NAMES))
            m.set_weights(init_weights(m.spec, seed=0))
            lis = Listener(model=m, classes_path=os.path.join(tmp, "classes.txt"), input_wav=paths[0], chunk_size=1024, scan_tile=args.tile)
            if int8:
                dm = m._device()
                clips = (torch.randn((512, pr.max_samples), device="cuda") * (3000 / 32768.0))
                lis.quantized = quantized_class(model_type).from_model(dm, calibrate(dm, Featurizer(pr)(clips)), "max")

            def run_loop():
                for p in paths:
                    lis._sb = lis.batch(1)                       # every file starts from a fresh stream
                    lis.input_wav = p
                    lis.run_wav(quiet=True)

            def run_scan():
                lis.scan_wav(paths, quiet=True)

            pcm = [lis._read_wav(p) for p in paths]
            run_scan()                                           # warm-up: kernels loaded, workspaces and caches allocated
            if args.scan_only:
                for _ in range(args.rounds):
                    run_scan()
                continue
            lis.input_wav = paths[0]
            lis._sb = lis.batch(1)
            chunk = pcm[0][:1024].tobytes()
            for _ in range(50):                                  # warm-up of the chunk loop
                lis.step(chunk)
            t_loop, t_scan = [], []
            for _ in range(args.rounds):                         # alternating
                t_loop.append(wall(run_loop))
                t_scan.append(wall(run_scan))
            stages = {}
            for _ in range(max(3, args.rounds)):
                tm = {}
                t_dev = wall(lambda: scan(pr, m._device(), pcm, chunk_size=1024, class_names=NAMES, decoder=lis.threshold_decoder,
                                          quantized=lis.quantized, tile=args.tile, timings=tm))
                stages.setdefault("scan_call_wall_ms", []).append(t_dev * 1e3)
                for k, evs in tm.items():
                    stages.setdefault(k + "_ms", []).append(sum(a.elapsed_time(b) for a, b in evs))
            rec = {"workload": tag, "files": files, "audio_seconds": audio_s, "model": model_type + ("_int8" if int8 else ""), "tile": args.tile,
                   "rounds": args.rounds, "run_wav_s": t_loop, "scan_wav_s": t_scan,
                   "run_wav_median_s": statistics.median(t_loop), "scan_wav_median_s": statistics.median(t_scan),
                   "stages_median_ms": {k: statistics.median(v) for k, v in stages.items()}}
            rec["speedup"] = rec["run_wav_median_s"] / rec["scan_wav_median_s"]
            rec["run_wav_x_real_time"] = audio_s / rec["run_wav_median_s"]
            rec["scan_wav_x_real_time"] = audio_s / rec["scan_wav_median_s"]
            rec["scan_device_x_real_time"] = audio_s / (rec["stages_median_ms"]["scan_call_wall_ms"] / 1e3)
            records.append(rec)
            st = rec["stages_median_ms"]
            print("%-8s %-20s run_wav %8.3f s (%7.0f x real time)  scan_wav %7.4f s (%9.0f x)  speed-up %6.1f x | scan() %7.2f ms: rows %.2f gather %.2f "
                  "forward %.2f scan %.2f" % (tag, rec["model"], rec["run_wav_median_s"], rec["run_wav_x_real_time"], rec["scan_wav_median_s"],
                                              rec["scan_wav_x_real_time"], rec["speedup"], st["scan_call_wall_ms"], st.get("rows_ms", 0),
                                              st.get("gather_ms", 0), st.get("forward_ms", 0), st.get("scan_ms", 0)), flush=True)
        for p in paths:
            os.remove(p)
    if args.out and records:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
