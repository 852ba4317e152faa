"""The transfer path in figures (kws_model_embed, kws_head_fit):

  embed      kws_model_embed against kws_model_forward at a batch of 4096 clips, for the four model kinds;
  one job    one head, N = 100 000 embeddings, E = 128, C = 12, batch = 64, one epoch (1563 steps): the kernel's own time (the library's
             per-launch timing), the fit_heads call from Python (uploads of order / labels and the final synchronisation included), and
             the same steps written with torch operators on the same device (matmul, softmax, the loss's gradient, Adam by hand), whose
             final weights are compared with the kernel's before anything is timed;
  many jobs  J = 1, 256 and 4096 independent small jobs (32 steps of 64 rows each) in one launch: head-steps per second.

A single job occupies one of the chip's compute units and is latency bound; what it can gain over the torch loop is launch and host
overhead only.  The tool reports, it asserts no ratio.

    python tools/transferbench.py [--rounds 7] [--out profiles/transferbench.json]

Every figure is the median of --rounds repetitions after warm-up runs of the same work.  The last line printed is the record as one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import numpy as np
import torch

from kws_amd import lib as _l
from kws_amd import transfer as T

BATCH_CLIPS = 4096
N, E, C, BATCH = 100000, 128, 12, 64
SMALL_STEPS = 32


def event_ms(fn, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall_ms(fn, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_ms(fn, rounds, name="head_fit_kernel"):
    out = []
    for _ in range(rounds):
        _l.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        rep = _l.prof_report()
        _l.prof_enable(False)
        out.append(rep[name]["total_ms"])
    return out


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def embed_cases(rounds):
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    cases = []
    f = torch.randn((BATCH_CLIPS, pr.n_features, pr.feature_size), device="cuda")
    for kind in ("simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"):
        m = get_model(kind, C)
        m.set_weights(init_weights(m.spec, seed=0))
        dm = m._device()
        for _ in range(3):
            dm.forward(f, True, False)
            dm.embed(f)
        t_f, t_e = [], []
        for _ in range(rounds):                                 # alternating
            t_f += event_ms(lambda: dm.forward(f, True, False), 1)
            t_e += event_ms(lambda: dm.embed(f), 1)
        cases.append({"model": kind, "clips": BATCH_CLIPS, "forward_ms": med(t_f), "embed_ms": med(t_e)})
        print("%-16s forward %.3f ms, embed %.3f ms at %d clips" % (kind, cases[-1]["forward_ms"]["median"], cases[-1]["embed_ms"]["median"],
                                                                    BATCH_CLIPS), flush=True)
    return cases


def torch_epoch(emb, y, order, k0, b0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """the steps of one kws_head_fit job from torch operators (plain loss, Adam)"""
    W, b = k0.clone(), b0.clone()
    mW, vW, mb, vb = torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(b)
    n = order.numel()
    t = 0
    for s in range(0, n, BATCH):
        rows = order[s:s + BATCH]
        x, yy = emb.index_select(0, rows), y.index_select(0, rows)
        p = torch.softmax(x @ W + b, 1)
        py = p.gather(1, yy[:, None])
        live = ((py >= 1e-7) & (py <= 1 - 1e-7)).float()
        d = p.scatter_add(1, yy[:, None], -torch.ones_like(py)) * live / rows.numel()
        gW, gb = x.t() @ d, d.sum(0)
        t += 1
        lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
        for w_, g_, m_, v_ in ((W, gW, mW, vW), (b, gb, mb, vb)):
            m_.mul_(b1).add_(g_, alpha=1 - b1)
            v_.mul_(b2).addcmul_(g_, g_, value=1 - b2)
            w_.addcdiv_(m_, v_.sqrt().add_(eps), value=-lr_t)
    return W, b


def one_job(rounds):
    rng = np.random.default_rng(0)
    emb = torch.from_numpy(np.clip(rng.normal(-0.2, 1.0, (N, E)), 0.0, 6.0).astype(np.float32)).cuda()
    y = rng.integers(0, C, N)
    order = rng.permutation(N).astype(np.int32)
    k0, b0 = T.glorot_head(E, C, 0)
    job = dict(order=order, num_classes=C, batch_size=BATCH, init=(k0, b0))
    y_d, order_d = torch.from_numpy(y).cuda(), torch.from_numpy(order.astype(np.int64)).cuda()
    k0_d, b0_d = torch.from_numpy(k0).cuda(), torch.from_numpy(b0).cuda()
    head = T.fit_heads(emb, y, [job])[0]
    Wt, bt = torch_epoch(emb, y_d, order_d, k0_d, b0_d)
    diff = float((Wt - torch.from_numpy(head.kernel).cuda()).abs().max())
    steps = -(-N // BATCH)
    t_k, t_c, t_t = [], [], []
    for _ in range(rounds):
        t_k += kernel_ms(lambda: T.fit_heads(emb, y, [job]), 1)
        t_c += wall_ms(lambda: T.fit_heads(emb, y, [job]), 1)
        t_t += wall_ms(lambda: torch_epoch(emb, y_d, order_d, k0_d, b0_d), 1)
    rec = {"N": N, "E": E, "C": C, "batch": BATCH, "steps": steps, "kernel_ms": med(t_k), "fit_heads_call_ms": med(t_c),
           "torch_loop_ms": med(t_t), "kernel_us_per_step": statistics.median(t_k) * 1e3 / steps,
           "torch_us_per_step": statistics.median(t_t) * 1e3 / steps, "max_abs_weight_difference_to_torch": diff}
    print("one job, %d steps: kernel %.2f ms (%.2f us per step), fit_heads call %.2f ms, torch loop %.1f ms (%.1f us per step); "
          "weights differ by at most %.2g" % (steps, rec["kernel_ms"]["median"], rec["kernel_us_per_step"], rec["fit_heads_call_ms"]["median"],
                                              rec["torch_loop_ms"]["median"], rec["torch_us_per_step"], diff), flush=True)
    return rec, emb, y


def many_jobs(emb, y, rounds):
    rng = np.random.default_rng(1)
    out = []
    for J in (1, 256, 4096):
        jobs = [dict(order=rng.integers(0, N, SMALL_STEPS * BATCH).astype(np.int32), num_classes=C, batch_size=BATCH, seed=j) for j in range(J)]
        T.fit_heads(emb, y, jobs)
        t_k = kernel_ms(lambda: T.fit_heads(emb, y, jobs), rounds)
        k = statistics.median(t_k)
        out.append({"jobs": J, "steps_per_job": SMALL_STEPS, "batch": BATCH, "E": E, "C": C, "kernel_ms": med(t_k),
                    "head_steps_per_s": J * SMALL_STEPS / (k * 1e-3)})
        print("J %5d x %d steps: kernel %.3f ms, %.3g head-steps per second" % (J, SMALL_STEPS, k, out[-1]["head_steps_per_s"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "conditions": "warm-up runs of the same work first, then the median of `rounds` repetitions (min and max kept); "
                            "embed / forward and kernel / call / torch repetitions alternate",
              "build_id": {k: _l.build_id().get(k) for k in ("kws_transfer.hip", "kws_model.hip", "kws_rnn.hip")}}
    record["embed"] = embed_cases(args.rounds)
    record["one_job"], emb, y = one_job(args.rounds)
    record["many_jobs"] = many_jobs(emb, y, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
