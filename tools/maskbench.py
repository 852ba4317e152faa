"""Cost of the feature-mask stage (kws_amd.augment.FeatureMask, kws_feature_mask) at B = 4096 and the default 30 x 20 features:
  1. the stage's kernel alone, in place, per configuration (rate 1.0 and 0.5, zero and mean fill, with and without warp): many
     back-to-back launches per sample between two events, several rounds with the configurations alternating, medians and the rounds;
     next to every time the share of the stage's HBM floor 2 B T F 4 bytes at 8 TB/s it reaches;
  2. the pipelined simple_cnn fit step on raw audio (tools/fitprof.py's workload) without and with the default FeatureMask, alternating
     in one process;
  3. with --parent-lib: the mask-off fit step of a child process per build (the given build of libkws_hip.so, e.g. the parent
     commit's, and the in-tree one, alternating), and the bench.py step of both through tools/ab_libs.py.
Prints one JSON line; --out also writes it to a file.

    python tools/maskbench.py [--rounds 5] [--parent-lib other/libkws_hip.so] [--out profiles/specaug_bench.json] [--kernel-only]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

HBM_GBS = 8000.0          # MI355X HBM3E peak


def stat(v):
    import numpy as np
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "rounds": [round(x, 4) for x in v]}


def time_ms(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def fit_steps(torch, variants, rounds, clips):
    """ms per step of whole fit epochs (wall time / steps) for every (name, fit keywords), alternating within each round"""
    import bench
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    B, C = 4096, 36
    nb = max(1, clips // B)
    wav_np, lab_np = bench.synthetic_batch(B, 0, C)
    x = torch.from_numpy(wav_np).cuda().repeat(nb, 1)
    y = torch.from_numpy(lab_np).cuda().repeat(nb)
    m = KWSModel("simple_cnn", C, seed=0)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    for _, kw in variants:
        m.fit(x, y, batch_size=B, epochs=1, verbose=0, **kw)
    st = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, kw in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x, y, batch_size=B, epochs=1, verbose=0, **kw)
            torch.cuda.synchronize()
            st[n].append((time.perf_counter() - t0) * 1e3 / nb)
    return st


def child(lib, rounds, clips):
    cmd = [sys.executable, os.path.abspath(__file__), "--fit-only", "--lib", lib, "--rounds", str(rounds), "--fit_clips", str(clips)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("fit child on %s failed: %s" % (lib, out.stderr[-800:]))
    return json.loads(out.stdout.strip().splitlines()[-1])["plain"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--fit_clips", type=int, default=4096 * 24)
    ap.add_argument("--parent-lib", default=None, help="another build of libkws_hip.so (the parent commit's) for the mask-off A/B")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="only launch the stage's kernel (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--fit-only", action="store_true", help="only the mask-off fit step, on --lib ('-': the in-tree build)")
    ap.add_argument("--lib", default="-")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.fit_only and args.lib != "-":
        import foreign_lib
        foreign_lib.use(args.lib)
    import torch
    torch.manual_seed(0)
    if args.fit_only:
        st = fit_steps(torch, (("plain", {}),), args.rounds, args.fit_clips)
        print(json.dumps({"lib": args.lib, "plain": st["plain"]}))
        return
    from kws_amd.augment import FeatureMask
    B, T, F = 4096, 30, 20
    kern = {"rate1.0_mean": FeatureMask(seed=1), "rate1.0_zero": FeatureMask(fill="zero", seed=1),
            "rate0.5_mean": FeatureMask(rate=0.5, seed=1), "rate0.5_zero": FeatureMask(rate=0.5, fill="zero", seed=1),
            "rate1.0_mean_warp5": FeatureMask(warp=5, seed=1), "rate1.0_zero_warp5": FeatureMask(warp=5, fill="zero", seed=1),
            "rate0.5_mean_warp5": FeatureMask(warp=5, rate=0.5, seed=1)}
    feat = torch.empty((B, T, F), device="cuda").uniform_(-60.0, 20.0)
    step = [0]

    def run(fm):
        step[0] += 1
        fm(feat, step[0], out=feat)

    if args.kernel_only:
        for _ in range(args.iters):
            for fm in kern.values():
                run(fm)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": len(kern) * args.iters, "order": list(kern)}))
        return

    floor_bytes = 2 * B * T * F * 4
    res = {"B": B, "n_features": T, "feature_size": F, "in_place": True, "launches_per_sample": args.iters,
           "hbm_floor": {"bytes": floor_bytes, "ms": round(floor_bytes / (HBM_GBS * 1e6), 5)}, "kernel": {}}
    kt = {n: [] for n in kern}
    for _ in range(args.rounds):
        for n, fm in kern.items():
            kt[n].append(time_ms(torch, lambda: run(fm), args.iters))
    for n in kern:
        res["kernel"][n] = stat(kt[n])
        res["kernel"][n]["share_of_hbm_floor"] = round(res["hbm_floor"]["ms"] / res["kernel"][n]["median_ms"], 4)
    res["kernel"]["note"] = ("event time of %d back-to-back launches / %d: launch gaps included; share_of_hbm_floor = (2 B T F 4 bytes / 8 TB/s) / "
                             "median, although a clip that is not applied moves no bytes in place" % (args.iters, args.iters))

    st = fit_steps(torch, (("plain", {}), ("feature_mask", {"feature_mask": FeatureMask(seed=1)})), args.rounds, args.fit_clips)
    res["fit_step"] = {n: stat(v) for n, v in st.items()}
    res["fit_step"]["note"] = "wall time of a whole fit epoch / steps (includes the epoch's host bookkeeping and one device sync); raw audio, simple_cnn"
    res["device"] = torch.cuda.get_device_name(0)

    def emit():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    emit()                                                   # the A/B below takes minutes: what is measured so far is kept

    if args.parent_lib:
        ab = {"parent": [], "in_tree": []}
        for _ in range(args.ab_rounds):
            for name, lib in (("parent", args.parent_lib), ("in_tree", "-")):
                ab[name] += child(lib, 2, args.fit_clips)
        res["fit_step_mask_off_vs_parent"] = {n: stat(v) for n, v in ab.items()}
        res["fit_step_mask_off_vs_parent"]["note"] = "one process per build and round, builds alternating, two timed epochs each; no FeatureMask object exists"
        emit()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_libs.py"), str(args.ab_rounds), args.parent_lib, "-"],
                             capture_output=True, text=True, timeout=1500)
        rows = {"parent": [], "in_tree": []}
        for line in out.stdout.splitlines():
            w = line.split()
            if len(w) >= 3 and w[0] in (args.parent_lib, "-"):
                rows["parent" if w[0] == args.parent_lib else "in_tree"].append(float(w[2]))
        if not rows["parent"] or not rows["in_tree"]:
            raise RuntimeError("tools/ab_libs.py printed no result: %s %s" % (out.stdout[-500:], out.stderr[-500:]))
        res["bench_step_vs_parent"] = {n: stat(v) for n, v in rows.items()}
        res["bench_step_vs_parent"]["note"] = "tools/ab_libs.py: bench.py --full --steps 300 --no-cpu-baseline --no-extra, one process per run, ms per step"
    print(json.dumps(res))
    emit()


if __name__ == "__main__":
    main()
