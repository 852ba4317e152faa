"""Cost of the optimizer options (kws_optimizer_step, include/kws.h) on the simple_cnn parameter buffer (134 932 floats) against the
plain Adam kernel (kws_adam_step): plain Adam, Adam with clipnorm, SGD with momentum and global_clipnorm, centered RMSprop with momentum.
Each variant runs --steps back-to-back steps between two device events after a warm-up; variants alternate within each of --rounds rounds
and the medians are reported.  These times include the host's launch cost per step; the kernels' own durations and the kernel count per
step come from a separate `rocprofv3 --kernel-trace --stats` run of --kernel-only.  Prints one JSON line; --out also writes it to a file.

--averaging measures the weight-averaging wrappers instead (MovingAverage, SWA, Lookahead over Adam, SGD with momentum and centered
RMSprop).  Per optimizer: the step without a wrapper; that step followed by a separate torch lerp_ of an average towards the parameters
(what the fusion replaces); and the step under each wrapper.  MovingAverage folds the slot into every step, SWA and Lookahead (periods
10 and 6, the reference's) into one step of their period.

    python tools/optbench.py [--rounds 7] [--steps 200] [--out optbench.json] [--kernel-only] [--averaging]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def variants():
    from common import model_utils as mu
    return [("adam_plain", None),
            ("adam_clipnorm", mu.Adam(1e-3, clipnorm=1.0)),
            ("sgd_momentum_global_clipnorm", mu.SGD(0.01, momentum=0.9, global_clipnorm=1.0)),
            ("rmsprop_centered_momentum", mu.RMSprop(1e-3, momentum=0.9, centered=True))]


def averaging_variants():
    """[(name, inner optimizer factory, wrapper name or None, lerp after the step)]"""
    from common import model_utils as mu
    inner = [("adam", lambda: mu.Adam(1e-3)), ("sgd_momentum", lambda: mu.SGD(0.01, momentum=0.9)),
             ("rmsprop_centered", lambda: mu.RMSprop(1e-3, centered=True))]
    out = []
    for name, make in inner:
        out.append((name + "/plain", make, None, False))
        out.append((name + "/plain_then_lerp", make, None, True))
        for w in ("ema", "swa", "lookahead"):
            out.append((name + "/" + w, make, w, False))
    return out


def averaging_steps(spec, rng):
    from common import model_utils as mu
    from kws_amd.model import DeviceModel
    models = {}
    for name, make, wrapper, lerp in averaging_variants():
        dm = DeviceModel(spec)
        dm.params[:spec.param_count].copy_(torch.from_numpy((0.1 * rng.standard_normal(spec.param_count)).astype(np.float32)))
        dm.grads[:spec.param_count].copy_(torch.from_numpy((0.01 * rng.standard_normal(spec.param_count)).astype(np.float32)))
        opt = mu.get_averaged_optimizer(wrapper, make())
        avg = dm.params.clone() if lerp else None

        def step(dm=dm, opt=opt, avg=avg):
            dm.optimizer_step(opt, 1e-3)
            opt.iterations += 1                 # the wrappers' schedules run on the update count
            if avg is not None:
                avg.lerp_(dm.params, 0.01)
        step()
        models[name] = step
    return models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--averaging", action="store_true", help="measure the weight-averaging wrappers instead of the optimizer options")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="run each variant --steps times and exit (for rocprofv3)")
    a = ap.parse_args()
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", 36, 30, 20)
    rng = np.random.default_rng(0)
    models = averaging_steps(spec, rng) if a.averaging else {}
    for name, opt in ([] if a.averaging else variants()):
        dm = DeviceModel(spec)
        dm.params[:spec.param_count].copy_(torch.from_numpy((0.1 * rng.standard_normal(spec.param_count)).astype(np.float32)))
        dm.grads[:spec.param_count].copy_(torch.from_numpy((0.01 * rng.standard_normal(spec.param_count)).astype(np.float32)))
        step = (lambda dm=dm: dm.adam_step(1e-3)) if opt is None else (lambda dm=dm, opt=opt: dm.optimizer_step(opt, 1e-3))
        step()                                  # warm-up: slots and the workspace are created here
        models[name] = step
    torch.cuda.synchronize()
    if a.kernel_only:
        for name, step in models.items():
            for _ in range(a.steps):
                step()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "steps_per_variant": a.steps, "variants": list(models)}))
        return
    times = {name: [] for name in models}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, step in models.items():
            for _ in range(10):
                step()
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    res = {"params": spec.param_count, "rounds": a.rounds, "steps": a.steps,
           "us_per_step_median": {k: round(float(np.median(v)), 2) for k, v in times.items()},
           "us_per_step_min": {k: round(float(np.min(v)), 2) for k, v in times.items()},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
