"""kws_score_hist against the torch-operator composition of the same counts, on the same device: a one-hot mask, a bin index and
bincount for the histograms, a gather and a comparison for the rank, a row maximum for the calibration counts.  Two batch sizes (the
evaluation's batch of 4096 clips and a scan's windows, --clips) times two class counts (--classes and 35); per case the kernel's own
time (the library's per-launch timing), the composition's and the kernel call's time between device events, the GB/s over the
B * C * 4 + B * 4 bytes the statistics must read and that rate's fraction of the HBM roofline, and next to them the time of the
simple_cnn forward pass that produces a batch of such scores.  Both forms are checked to give the same integers before they are timed.

    python tools/scorebench.py [--clips 1048576] [--classes 12] [--bins 1024] [--rounds 20] [--out profiles/score_hist_bench.json]

The last line printed is the record as one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import torch

from kws_amd import lib as _l
from kws_amd.metrics import ScoreStats, uses_lds

HBM_BYTES_PER_S = 8e12        # the spec figure the fraction is taken of; a float4 copy reaches 6.3e12 on this part
EVAL_BATCH = 4096


def torch_counts(p, y, bins, hist, rank_counts, calib):
    """the same three arrays from torch operators (accumulating)"""
    B, C = p.shape
    valid = (y >= 0) & (y < C)
    p, y = p[valid], y[valid].long()
    b = (p * float(bins)).to(torch.int64).clamp_(0, bins - 1)
    b = torch.where(p >= 1, torch.full_like(b, bins - 1), b)
    b = torch.where(p > 0, b, torch.zeros_like(b))
    cls = torch.arange(C, device=p.device)[None, :]
    onehot = cls == y[:, None]
    hist += torch.bincount(((cls * 2 + onehot) * bins + b).reshape(-1), minlength=C * 2 * bins).view(C, 2, bins)
    py = p.gather(1, y[:, None])
    rank = ((p > py) | ((p == py) & (cls < y[:, None]))).sum(1)
    rank = torch.where(torch.isnan(p).any(1), torch.full_like(rank, C - 1), rank)
    rank_counts += torch.bincount(rank, minlength=C)
    top = b.max(1).values
    calib[0] += torch.bincount(top, minlength=bins)
    calib[1] += torch.bincount(top[rank == 0], minlength=bins)


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


def kernel_ms(fn, rounds):
    out = []
    for _ in range(rounds):
        _l.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        rep = _l.prof_report()
        _l.prof_enable(False)
        out.append(rep["score_hist_kernel"]["total_ms"])
    return out


def forward_ms(C, rounds):
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    m = get_model("simple_cnn", C)
    m.set_weights(init_weights(m.spec, seed=0))
    dm = m._device()
    f = torch.randn((EVAL_BATCH, pr.n_features, pr.feature_size), device="cuda")
    for _ in range(3):
        dm.forward(f, True, False)
    return statistics.median(event_ms(lambda: dm.forward(f, True, False), rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1048576)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(3)
    record = {"device": torch.cuda.get_device_name(0), "bins": args.bins, "rounds": args.rounds, "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "build_id": {"kws_score.hip": _l.build_id().get("kws_score.hip")}, "cases": []}
    for C in sorted({args.classes, 35}):
        fwd = forward_ms(C, args.rounds)
        for B in sorted({EVAL_BATCH, args.clips}):
            p = torch.softmax(3.0 * torch.randn((B, C), generator=gen, device="cuda"), 1)      # peaked, as a trained model's scores
            y = torch.randint(0, C, (B,), generator=gen, device="cuda", dtype=torch.int32)
            mine, ref = ScoreStats(C, args.bins), ScoreStats(C, args.bins)
            for _ in range(3):                                                                  # warm-up of both forms
                mine.update(p, y)
                torch_counts(p, y, args.bins, ref.hist, ref.rank_counts, ref.calib)
            same = all(bool((a == b).all()) for a, b in zip((mine.hist, mine.rank_counts, mine.calib), (ref.hist, ref.rank_counts, ref.calib)))
            if not same:
                raise SystemExit("kws_score_hist and the torch composition disagree at B %d, C %d" % (B, C))
            t_kernel, t_call, t_torch = [], [], []
            for _ in range(args.rounds):                                                        # alternating
                t_kernel += kernel_ms(lambda: mine.update(p, y), 1)
                t_call += event_ms(lambda: mine.update(p, y), 1)
                t_torch += event_ms(lambda: torch_counts(p, y, args.bins, ref.hist, ref.rank_counts, ref.calib), 1)
            k, c, t = statistics.median(t_kernel), statistics.median(t_call), statistics.median(t_torch)
            nbytes = B * C * 4 + B * 4
            case = {"clips": B, "classes": C, "lds_path": uses_lds(C, args.bins), "bytes_read": nbytes,
                    "kernel_ms": k, "kernel_ms_min_max": [min(t_kernel), max(t_kernel)], "call_ms": c,
                    "torch_ms": t, "torch_ms_min_max": [min(t_torch), max(t_torch)], "torch_over_kernel": t / k,
                    "kernel_gb_per_s": nbytes / (k * 1e-3) / 1e9, "fraction_of_hbm_roofline": nbytes / (k * 1e-3) / HBM_BYTES_PER_S,
                    "forward_ms_per_%d_clips" % EVAL_BATCH: fwd, "forward_ms_for_these_clips": fwd * B / EVAL_BATCH}
            record["cases"].append(case)
            print("B %8d C %3d: kernel %.4f ms (%.1f GB/s, %.3f of the HBM roofline), call %.4f ms, torch composition %.3f ms (%.1f x), "
                  "forward of these clips %.3f ms" % (B, C, k, case["kernel_gb_per_s"], case["fraction_of_hbm_roofline"], c, t, t / k,
                                                      case["forward_ms_for_these_clips"]), flush=True)
            del p, y, mine, ref
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
