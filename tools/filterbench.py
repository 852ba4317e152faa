"""Cost of the Butterworth filter augmentation (kws_amd.augment: FilterBank, WaveAugment.filter) at B = 4096: the filter kernel alone
(lowpass and bandpass banks, rates 1.0 and 0.5), featurize plain / filter / filter + noise / reverb + filter + noise, and the pipelined
simple_cnn fit step plain / filter + noise / reverb + filter + noise.  Variants alternate within each round (several rounds, medians).
Next to every kernel time stand its byte and FLOP counts and the HBM and VALU floors.  Kernel-only times for DESIGN.md come from a
separate `rocprofv3 --kernel-trace --stats` run of `--kernel-only`.  Prints one JSON line; --out also writes it to a file.

    python tools/filterbench.py [--rounds 5] [--out filterbench.json] [--kernel-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_GBS = 6300.0          # MI355X HBM3E, measured copy bandwidth
VALU_TFLOPS = 157.0       # fp32 vector peak (FMA = 2 FLOP)


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


def floors(B, filtered, ms, sections, padlen):
    """bytes, FLOP and the two floors (ms) of one filter launch with `filtered` of B clips filtered by `sections`-section designs"""
    nbytes = B * ms * 4 * 2                               # clip in + row out; the forward output and the rescale pass stay in the caches
    # 9 FLOP per section and sample (4 FMA + 1 mul), over the padded clip, twice per pass (zero-state run and rerun), two passes
    flop = filtered * (ms + 2 * padlen) * 4 * sections * 9
    return {"bytes": int(nbytes), "flop": int(flop),
            "hbm_floor_ms": round(nbytes / (HBM_GBS * 1e6), 4),
            "valu_floor_ms": round(flop / (VALU_TFLOPS * 1e9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--fit_clips", type=int, default=4096 * 12)
    ap.add_argument("--kernel-only", action="store_true", help="only launch the filter kernel (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from classifier.params import pr
    from kws_amd.augment import FilterBank, NoiseBank, RirBank, WaveAugment, random_filters, simulate_rirs
    from kws_amd.featurizer import Featurizer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    B, ms = 4096, pr.max_samples
    lp = FilterBank(random_filters(32, types=("lowpass",), seed=0))           # order 4: 2 sections, padlen 15
    bp = FilterBank(random_filters(32, types=("bandpass",), seed=0))          # order 4: 4 sections, padlen 27
    rirs = RirBank(simulate_rirs(32, seed=0))
    noise = NoiseBank([(0.1 * rng.standard_normal(960000 + 1000 * k)).astype(np.float32) for k in range(6)])
    kern = {"lp_1.0": WaveAugment(None, filters=lp, filter_rate=1.0, seed=1), "lp_0.5": WaveAugment(None, filters=lp, filter_rate=0.5, seed=1),
            "bp_1.0": WaveAugment(None, filters=bp, filter_rate=1.0, seed=1), "bp_0.5": WaveAugment(None, filters=bp, filter_rate=0.5, seed=1)}
    nz = WaveAugment(noise, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1)
    fn = WaveAugment(noise, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1, filters=bp, filter_rate=1.0)
    rfn = WaveAugment(noise, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1, rirs=rirs, reverb_rate=1.0, filters=bp, filter_rate=1.0)
    wav = (0.1 * torch.randn((B, ms), device="cuda")).contiguous()
    scratch = torch.empty((B, ms), device="cuda")
    lens = torch.empty((B,), dtype=torch.int32, device="cuda")
    res = {"B": B, "filters": len(bp), "kernel": {}, "featurize": {}}

    if args.kernel_only:
        for _ in range(args.iters):
            for a in kern.values():
                a.filter(wav, step=1, out=scratch, lengths=lens, filter_used=False)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": len(kern) * args.iters}))
        return

    kt = {n: [] for n in kern}
    for _ in range(args.rounds):
        for n, a in kern.items():
            kt[n].append(time_ms(lambda: a.filter(wav, step=1, out=scratch, lengths=lens, filter_used=False), args.iters))
    for n, a in kern.items():
        t = float(np.median(kt[n]))
        filtered = B if a.filter_rate == 1.0 else B // 2
        fb = a.filters
        res["kernel"][n] = dict(floors(B, filtered, ms, fb.n_sections, int(fb.padlen.max())), median_ms=round(t, 4),
                                rounds=[round(x, 4) for x in kt[n]])

    f = Featurizer(pr)
    out = torch.empty((B, pr.n_features, pr.feature_size), device="cuda")
    variants = (("plain", None), ("filter", kern["bp_1.0"]), ("noise", nz), ("filter_noise", fn), ("reverb_filter_noise", rfn))
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
    fits = (("plain", {}), ("filter_noise", {"augment": fn}), ("reverb_filter_noise", {"augment": rfn}))
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
