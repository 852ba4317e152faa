"""Cost of the tempo and pitch perturbation (kws_amd.augment: WaveAugment.pitch_perturb) at B = 4096, the default geometry (1 s clips at
16 kHz, n_fft 512, the default 16 x 512 table) and int16 input: the stage's two kernels in three configurations (tempo only, pitch only,
both; every clip perturbed), the same call at several workspace sizes (does a tile that fits the Infinity Cache pay?), and the pipelined
simple_cnn fit step on raw audio without and with the stage.  Variants alternate within each round (several rounds, medians and the
rounds themselves).  Next to every kernel time stands the HBM floor of the bytes the two kernels move.  Run tools/speedbench.py in the
same session as the yardstick.  Prints one JSON line; --out also writes it to a file.

    python tools/pitchbench.py [--rounds 5] [--out pitchbench.json] [--no-fit]"""
import argparse
import json
import math
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


def call_clip_bytes(N, ms, rho_max, r_max, Z):
    """the workspace bytes of one clip in a call whose largest rho and r are these (csrc/kws_pitch.hip: slots)"""
    H = N // 4
    need = int(math.floor((ms - 1) * r_max)) + 2 + int(math.ceil(Z * max(r_max, 1.0)))
    jn = (need + N // 2 + H - 1) // H
    mn = int(math.floor((jn - 1) * rho_max)) + 2
    return (mn * (N // 2 + 1) + 15) // 16 * 16 * 8 + (need + 31) // 32 * 32 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tiles", default="16,32,64,128,256,512,1024", help="workspaces, in clips at the ranges' ends (kws_pitch_workspace_bytes)")
    ap.add_argument("--fit_clips", type=int, default=4096 * 12)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from classifier.params import pr
    from kws_amd.augment import PITCH_TILE_CLIPS, Resampler, WaveAugment, pitch_workspace_bytes
    torch.manual_seed(0)
    B, ms, N = 4096, pr.max_samples, 512
    rs = Resampler()
    kern = {"tempo": WaveAugment(None, tempo=(0.85, 1.2), pitch_n_fft=N, seed=1),
            "pitch": WaveAugment(None, pitch=(-2, 2), pitch_n_fft=N, resampler=rs, seed=1),
            "both": WaveAugment(None, tempo=(0.85, 1.2), pitch=(-2, 2), pitch_n_fft=N, resampler=rs, seed=1)}
    wav = (0.1 * torch.randn((B, ms), device="cuda") * 32768).clamp(-32768, 32767).to(torch.int16).contiguous()
    scratch = torch.empty((B, ms), device="cuda")
    lens = torch.empty((B,), dtype=torch.int32, device="cuda")
    tiles = [int(t) for t in args.tiles.split(",")]
    ws = torch.empty((pitch_workspace_bytes(N, ms, max(tiles + [PITCH_TILE_CLIPS])),), dtype=torch.uint8, device="cuda")
    one = pitch_workspace_bytes(N, ms, 1)
    r_lo, r_hi = float(np.float32(2.0 ** (-2.0 / 12.0))), float(np.float32(2.0 ** (2.0 / 12.0)))
    mine = call_clip_bytes(N, ms, float(np.float32(1.2)) / r_lo, r_hi, rs.zero_crossings)          # a clip of the "both" configuration
    frames, bins = 1 + ms // (N // 4), N // 2 + 1
    # per clip at rho = 1: the int16 source in, the spectrum out and in again, the float32 row out; a pitched clip's stretched signal
    # goes out and in once more
    floor = {"tempo": B * (2 * ms + 2 * 8 * frames * bins + 4 * ms)}
    floor["pitch"] = floor["both"] = floor["tempo"] + B * 8 * ms
    res = {"B": B, "max_samples": ms, "n_fft": N, "table": [rs.zero_crossings, rs.phases], "input": "int16", "tile_clips": PITCH_TILE_CLIPS,
           "workspace_bytes_per_clip": one, "both_bytes_per_clip": mine, "kernel": {}, "tiles": {},
           "hbm_floor": {n: {"bytes": b, "ms": round(b / (HBM_GBS * 1e6), 4)} for n, b in floor.items()}}

    def run(a, tile=PITCH_TILE_CLIPS):
        a.pitch_perturb(wav, step=1, max_samples=ms, out=scratch, lengths=lens, tempo_used=False, pitch_used=False, workspace=ws[:one * tile])

    kt = {n: [] for n in kern}
    tt = {t: [] for t in tiles}
    for _ in range(args.rounds):
        for n, a in kern.items():
            kt[n].append(time_ms(lambda: run(a), args.iters))
        for t in tiles:
            tt[t].append(time_ms(lambda: run(kern["both"], t), args.iters))
    for n in kern:
        res["kernel"][n] = {"median_ms": round(float(np.median(kt[n])), 4), "rounds": [round(x, 4) for x in kt[n]]}
    for t in tiles:
        res["tiles"][str(t)] = {"median_ms": round(float(np.median(tt[t])), 4), "rounds": [round(x, 4) for x in tt[t]],
                                "workspace_mb": round(one * t / 2 ** 20, 1), "clips_per_tile": min(B, one * t // mine)}
    from kws_amd import lib as _l
    _l.prof_enable(True)
    run(kern["both"])
    torch.cuda.synchronize()
    res["both_kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in _l.prof_report().items() if k.startswith("pitch")}
    _l.prof_enable(False)
    del ws

    if not args.no_fit:
        from classifier.loss import SparseCategoricalCrossEntropy
        from classifier.model import KWSModel
        from common.model_utils import get_optimizer
        Nc, C = args.fit_clips, 36
        x = (0.1 * torch.randn((Nc, ms), device="cuda")).contiguous()
        y = torch.randint(0, C, (Nc,), device="cuda")
        m = KWSModel("simple_cnn", C, seed=0)
        m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
        steps = Nc // B
        fits = (("plain", {}), ("tempo_pitch", {"augment": kern["both"]}))
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
