"""Cost of the background-noise augmentation (kws_amd.augment): the augmented featurize (plan + fused featurizer) against the plain one at
B = 4096 for float32 and int16 audio, and the pipelined simple_cnn fit step with and without augmentation.  Variants alternate within
each round (several rounds, medians), so drift of the clock or of the neighbours hits both alike.  Prints one JSON line; --out also
writes it to a file.

    python tools/augbench.py [--rounds 5] [--out augbench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_GBS = 8000.0


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--fit_clips", type=int, default=4096 * 12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from classifier.params import pr
    from kws_amd.augment import NoiseBank, WaveAugment
    from kws_amd.featurizer import Featurizer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    B = 4096
    # a bank the size of Speech Commands' _background_noise_: six recordings of about a minute
    bank = NoiseBank([(0.1 * rng.standard_normal(960000 + 1000 * k)).astype(np.float32) for k in range(6)])
    aug = WaveAugment(bank, snr=(0, 5, 10, 20), noised_rate=0.8, seed=1)
    f = Featurizer(pr)
    wav32 = (0.1 * torch.randn((B, pr.max_samples), device="cuda")).contiguous()
    wav16 = (wav32 * 32768).to(torch.int16)
    out = torch.empty((B, pr.n_features, pr.feature_size), device="cuda")
    res = {"B": B, "featurize": {}}
    for name, w in (("f32", wav32), ("i16", wav16)):
        plain, augd, plan_only = [], [], []
        for _ in range(args.rounds):
            plain.append(time_ms(lambda: f(w, out=out), args.iters))
            augd.append(time_ms(lambda: f(w, out=out, augment=aug, step=1), args.iters))
            plan_only.append(time_ms(lambda: aug.plan(w, step=1), args.iters))
        sb = w.element_size()
        # bytes: the plain kernel reads every sample once and writes the features; augmented adds the plan's read of the voice head and
        # the noise window (one float32 per kept sample), the plan records (32 B) are noise
        plain_bytes = B * (pr.max_samples * sb + pr.n_features * pr.feature_size * 4)
        aug_bytes = plain_bytes + B * (pr.max_samples * sb + 0.8 * pr.max_samples * 4 + 64)
        p, a, q = float(np.median(plain)), float(np.median(augd)), float(np.median(plan_only))
        res["featurize"][name] = {"plain_ms": round(p, 4), "augmented_ms": round(a, 4), "plan_ms": round(q, 4), "ratio": round(a / p, 3),
                                  "plain_GBs": round(plain_bytes / p / 1e6, 1), "augmented_GBs": round(aug_bytes / a / 1e6, 1),
                                  "augmented_hbm_frac": round(aug_bytes / a / 1e6 / HBM_GBS, 4), "rounds_plain": [round(x, 4) for x in plain],
                                  "rounds_augmented": [round(x, 4) for x in augd]}

    # the pipelined simple_cnn fit step on a resident raw-audio set, plain and augmented, alternating
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    N, C = args.fit_clips, 36
    x = (0.1 * torch.randn((N, pr.max_samples), device="cuda")).contiguous()
    y = torch.randint(0, C, (N,), device="cuda")
    m = KWSModel("simple_cnn", C, seed=0)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    steps = N // B
    m.fit(x, y, batch_size=B, epochs=1, verbose=0)
    m.fit(x, y, batch_size=B, epochs=1, verbose=0, augment=aug)
    step_plain, step_aug = [], []
    for _ in range(args.rounds):
        for lst, kw in ((step_plain, {}), (step_aug, {"augment": aug})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x, y, batch_size=B, epochs=1, verbose=0, **kw)
            torch.cuda.synchronize()
            lst.append((time.perf_counter() - t0) * 1e3 / steps)
    sp, sa = float(np.median(step_plain)), float(np.median(step_aug))
    res["fit_step"] = {"B": B, "steps_per_epoch": steps, "plain_ms": round(sp, 4), "augmented_ms": round(sa, 4), "ratio": round(sa / sp, 4),
                       "rounds_plain": [round(v, 4) for v in step_plain], "rounds_augmented": [round(v, 4) for v in step_aug],
                       "note": "wall time of a whole fit epoch / steps (includes the epoch's host bookkeeping and one device sync)"}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
