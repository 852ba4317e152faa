"""Cost of the speed and loudness perturbation (kws_amd.augment: Resampler, WaveAugment.perturb) at B = 4096, the default geometry
(1 s clips at 16 kHz, the default 16 x 512 table) and int16 input: the stage's kernel alone in three configurations (speed only, loudness
only, both; every clip perturbed), and the pipelined simple_cnn fit step on raw audio without and with the stage.  Variants alternate
within each round (several rounds, medians and the rounds themselves).  Next to every kernel time stands the stage's HBM floor.
Kernel-only times for DESIGN.md come from a separate `rocprofv3 --kernel-trace --stats` run of `--kernel-only`.  Prints one JSON line;
--out also writes it to a file.

    python tools/speedbench.py [--rounds 5] [--out speedbench.json] [--kernel-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_GBS = 8000.0          # MI355X HBM3E peak


def time_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--fit_clips", type=int, default=4096 * 12)
    ap.add_argument("--kernel-only", action="store_true", help="only launch the stage's kernel (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from classifier.params import pr
    from kws_amd.augment import Resampler, WaveAugment
    torch.manual_seed(0)
    B, ms = 4096, pr.max_samples
    rs = Resampler()
    kern = {"speed": WaveAugment(None, speed=(0.9, 1.1), resampler=rs, seed=1),
            "loudness": WaveAugment(None, loudness=(-30, -15), seed=1),
            "both": WaveAugment(None, speed=(0.9, 1.1), loudness=(-30, -15), resampler=rs, seed=1)}
    wav = (0.1 * torch.randn((B, ms), device="cuda") * 32768).clamp(-32768, 32767).to(torch.int16).contiguous()
    scratch = torch.empty((B, ms), device="cuda")
    lens = torch.empty((B,), dtype=torch.int32, device="cuda")
    floor_bytes = 4 * (ms + ms) * B                          # 4 (Ls + max_samples) B: the source as float32 and the row out
    res = {"B": B, "max_samples": ms, "table": [rs.zero_crossings, rs.phases], "input": "int16", "kernel": {},
           "hbm_floor": {"bytes": floor_bytes, "ms": round(floor_bytes / (HBM_GBS * 1e6), 4)}}

    def run(a):
        a.perturb(wav, step=1, max_samples=ms, out=scratch, lengths=lens, speed_used=False, gain_used=False)

    if args.kernel_only:
        for _ in range(args.iters):
            for a in kern.values():
                run(a)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": len(kern) * args.iters, "order": list(kern)}))
        return

    kt = {n: [] for n in kern}
    for _ in range(args.rounds):
        for n, a in kern.items():
            kt[n].append(time_ms(lambda: run(a), args.iters))
    for n in kern:
        res["kernel"][n] = {"median_ms": round(float(np.median(kt[n])), 4), "rounds": [round(x, 4) for x in kt[n]]}

    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    N, C = args.fit_clips, 36
    x = (0.1 * torch.randn((N, ms), device="cuda")).contiguous()
    y = torch.randint(0, C, (N,), device="cuda")
    m = KWSModel("simple_cnn", C, seed=0)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    steps = N // B
    fits = (("plain", {}), ("speed_loudness", {"augment": kern["both"]}))
    for _, kw in fits:
        m.fit(x, y, batch_size=B, epochs=1, verbose=0, **kw)
    st = {n: [] for n, _ in fits}
    for _ in range(args.rounds):
        for n, kw in fits:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x, y, batch_size=B, epochs=1, verbose=0, **kw)
            torch.cuda.synchronize()
            st[n].append((time.perf_counter() - t0) * 1e3 / steps)
    res["fit_step"] = {n: {"median_ms": round(float(np.median(v)), 4), "rounds": [round(x, 4) for x in v]} for n, v in st.items()}
    res["fit_step"]["note"] = "wall time of a whole fit epoch / steps (includes the epoch's host bookkeeping and one device sync); float32 clips"
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
