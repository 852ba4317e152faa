"""Cost of the room-reverberation augmentation (kws_amd.augment: RirBank, WaveAugment.reverberate) at B = 4096: the reverb kernel alone
(every clip wet, and rate 0.5), featurize plain / noise / reverb / reverb + noise, and the pipelined simple_cnn fit step plain / noise /
reverb + noise.  Variants alternate within each round (several rounds, medians).  Next to every kernel time stand its byte and FLOP
counts and the three floors (HBM, VALU, LDS).  Kernel-only times for DESIGN.md come from a separate `rocprofv3 --kernel-trace --stats`
run of `--kernel-only`.  Prints one JSON line; --out also writes it to a file.

    python tools/reverbbench.py [--rounds 5] [--out reverbbench.json] [--kernel-only]"""
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
VALU_TFLOPS = 157.0       # fp32 vector peak (FMA = 2 FLOP)
LDS_BPC_CU, CUS, CLK_GHZ = 256.0, 256, 2.4
M = 16384                 # complex points of the packed 32768-point real transform


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


def floors(B, wet, ms):
    """bytes, FLOP and the three floors (ms) of one reverb launch with `wet` of B clips reverberated"""
    nbytes = B * ms * 4 * 2                               # clip in + row out; bank spectra and twiddles stay in the caches
    # per wet transform: 3 radix-16 passes (1024 DFT16 of ~144 real FLOP + 15 twiddle products of 6) + the radix-4 pass and the
    # spectrum step; two transforms per clip
    per_fft = 3 * 1024 * (144 + 15 * 6) + 4096 * (16 + 3 * 6)
    flop = wet * (2 * per_fft + M * 40)
    lds = wet * 7 * M * 8 * 2                             # 7 exchanges, every value written and read once (8 B complex)
    return {"bytes": int(nbytes), "flop": int(flop), "lds_bytes": int(lds),
            "hbm_floor_ms": round(nbytes / (HBM_GBS * 1e6), 4),
            "valu_floor_ms": round(flop / (VALU_TFLOPS * 1e9), 4),
            "lds_floor_ms": round(lds / (LDS_BPC_CU * CUS * CLK_GHZ * 1e6), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--fit_clips", type=int, default=4096 * 12)
    ap.add_argument("--kernel-only", action="store_true", help="only launch the reverb kernel (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from classifier.params import pr
    from kws_amd.augment import NoiseBank, RirBank, WaveAugment, simulate_rirs
    from kws_amd.featurizer import Featurizer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    B, ms = 4096, pr.max_samples
    rirs = RirBank(simulate_rirs(32, seed=0))
    noise = NoiseBank([(0.1 * rng.standard_normal(960000 + 1000 * k)).astype(np.float32) for k in range(6)])
    rv1 = WaveAugment(None, rirs=rirs, reverb_rate=1.0, seed=1)
    rv5 = WaveAugment(None, rirs=rirs, reverb_rate=0.5, seed=1)
    nz = WaveAugment(noise, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1)
    both = WaveAugment(noise, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1, rirs=rirs, reverb_rate=1.0)
    wav = (0.1 * torch.randn((B, ms), device="cuda")).contiguous()
    scratch = torch.empty((B, ms), device="cuda")
    lens = torch.empty((B,), dtype=torch.int32, device="cuda")
    res = {"B": B, "rirs": len(rirs), "kernel": {}, "featurize": {}}

    if args.kernel_only:
        for _ in range(args.iters):
            rv1.reverberate(wav, step=1, out=scratch, lengths=lens, rir_used=False)
            rv5.reverberate(wav, step=1, out=scratch, lengths=lens, rir_used=False)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": 2 * args.iters}))
        return

    k1, k5 = [], []
    for _ in range(args.rounds):
        k1.append(time_ms(lambda: rv1.reverberate(wav, step=1, out=scratch, lengths=lens, rir_used=False), args.iters))
        k5.append(time_ms(lambda: rv5.reverberate(wav, step=1, out=scratch, lengths=lens, rir_used=False), args.iters))
    for name, ts, wet in (("rate_1.0", k1, B), ("rate_0.5", k5, B // 2)):
        t = float(np.median(ts))
        res["kernel"][name] = dict(floors(B, wet, ms), median_ms=round(t, 4), rounds=[round(x, 4) for x in ts])

    f = Featurizer(pr)
    out = torch.empty((B, pr.n_features, pr.feature_size), device="cuda")
    variants = (("plain", None), ("noise", nz), ("reverb", rv1), ("reverb_noise", both))
    times = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, a in variants:
            times[n].append(time_ms(lambda: f(wav, out=out, augment=a, step=1), args.iters))
    for n, _ in variants:
        res["featurize"][n] = {"median_ms": round(float(np.median(times[n])), 4), "rounds": [round(x, 4) for x in times[n]]}

    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    N, C = args.fit_clips, 36
    x = (0.1 * torch.randn((N, ms), device="cuda")).contiguous()
    y = torch.randint(0, C, (N,), device="cuda")
    m = KWSModel("simple_cnn", C, seed=0)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    steps = N // B
    fits = (("plain", {}), ("noise", {"augment": nz}), ("reverb_noise", {"augment": both}))
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
    res["fit_step"]["note"] = "wall time of a whole fit epoch / steps (includes the epoch's host bookkeeping and one device sync)"
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
