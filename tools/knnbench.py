"""Nearest-neighbour search in figures (kws_knn, csrc/kws_knn.hip):

  self-search   every row of an (N, E) matrix of unit rows against all the others, N in {4096, 65536} x E in {48, 128}, k = 10;
  one query     one unit row against 65536 rows, E = 128, k = 10: the live-enrolment case, where the library cuts the reference rows
                into slices for different blocks and merges them.

Each time stands beside a torch baseline on the same GPU and data: torch.mm + torch.topk over chunks of at most 4096 queries, so that
at most 4096 x N scores exist at a time (the kernel never writes any).  Before anything is timed the two results are compared: the
record keeps the largest difference between the scores and the number of rows whose index sets differ.

For the kernel the tool reports the time of its launches alone (the library's per-launch timing: knn_kernel plus knn_merge_kernel), the
time of the whole kws_amd.neighbors.knn call between device events, 2 Q N E floating-point operations over the kernel time in TFLOP/s
and that rate's share of the 157.3 TFLOP/s float32 matrix peak of the MI355X.  The tool reports, it asserts no ratio.

    python tools/knnbench.py [--rounds 7] [--out profiles/knn_bench.json]

Every figure is the median of --rounds repetitions after warm-up runs of the same work, kernel and baseline alternating.  The last
line printed is the record as one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import numpy as np
import torch

from kws_amd import lib as _l
from kws_amd import neighbors as nb

PEAK_TFLOPS = 157.3
CHUNK = 4096
K = 10
SELF_CASES = [(4096, 48), (4096, 128), (65536, 48), (65536, 128)]
ONE_QUERY = (65536, 128)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(fn):
    _l.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    rep = _l.prof_report()
    _l.prof_enable(False)
    return sum(rep[n]["total_ms"] for n in ("knn_kernel", "knn_merge_kernel") if n in rep)


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def torch_knn(q, r, k, exclude_self):
    """chunked torch.mm + torch.topk: at most CHUNK x N scores at a time"""
    idx, score = [], []
    rt = r.t()
    for i in range(0, q.shape[0], CHUNK):
        s = torch.mm(q[i:i + CHUNK], rt)
        if exclude_self:
            n = s.shape[0]
            s[torch.arange(n, device=s.device), torch.arange(i, i + n, device=s.device)] = float("-inf")
        v, j = torch.topk(s, k, dim=1)
        idx.append(j)
        score.append(v)
    return torch.cat(idx), torch.cat(score)


def compare(got, want, k):
    """-> (largest score difference, number of rows whose index sets differ: torch sums in another order, so two references whose scores
    differ in the last bits may change places at the k-th rank)"""
    gi, gs = got
    wi, ws = want
    diff = float((gs - ws).abs().max())
    rows = (gi.long().sort(1)[0] != wi.sort(1)[0]).any(1)
    return diff, int(rows.sum())


def one_case(Q, N, E, exclude_self, rounds, rng):
    r = torch.from_numpy(rng.standard_normal((N, E)).astype(np.float32)).cuda()
    r = nb.normalize(r)[0]
    q = r if exclude_self else nb.normalize(torch.from_numpy(rng.standard_normal((Q, E)).astype(np.float32)).cuda())[0]
    ours = lambda: nb.knn(q, r, K, "dot", exclude_self=exclude_self)
    base = lambda: torch_knn(q, r, K, exclude_self)
    for _ in range(2):
        got, want = ours(), base()
    diff, rows = compare(got, want, K)
    t_k, t_c, t_b = [], [], []
    for _ in range(rounds):
        t_k.append(kernel_ms(ours))
        t_c.append(event_ms(ours))
        t_b.append(event_ms(base))
    flop = 2.0 * Q * N * E
    k_ms = statistics.median(t_k)
    rec = {"Q": Q, "N": N, "E": E, "k": K, "exclude_self": exclude_self, "slices": "the library's choice",
           "workspace_bytes": int(_l.get_lib().kws_knn_workspace_bytes(Q, N, E, K, 0)),
           "kernel_ms": med(t_k), "call_ms": med(t_c), "torch_ms": med(t_b),
           "kernel_tflops": flop / (k_ms * 1e-3) / 1e12, "kernel_share_of_fp32_matrix_peak": flop / (k_ms * 1e-3) / 1e12 / PEAK_TFLOPS,
           "torch_tflops": flop / (statistics.median(t_b) * 1e-3) / 1e12,
           "call_over_torch": statistics.median(t_c) / statistics.median(t_b),
           "max_abs_score_difference_to_torch": diff, "rows_with_other_index_sets": rows}
    print("Q %6d N %6d E %3d: kernel %8.3f ms (%.1f TFLOP/s, %.0f %% of the fp32 matrix peak), call %8.3f ms, torch mm + topk %8.3f ms; "
          "scores differ by at most %.2g, %d rows with other index sets"
          % (Q, N, E, k_ms, rec["kernel_tflops"], 100 * rec["kernel_share_of_fp32_matrix_peak"], rec["call_ms"]["median"],
             rec["torch_ms"]["median"], diff, rows), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "fp32_matrix_peak_tflops": PEAK_TFLOPS,
              "conditions": "two warm-up runs of the same work first (the results compared), then the median of `rounds` repetitions (min and "
                            "max kept); kernel, call and torch repetitions alternate; kernel_ms is the library's per-launch timing of "
                            "knn_kernel + knn_merge_kernel, call_ms and torch_ms are device events around the whole call; the rows are "
                            "unit rows, normalised outside the timed window",
              "build_id": {k: _l.build_id().get(k) for k in ("kws_knn.hip",)}}
    record["self_search"] = [one_case(N, N, E, True, args.rounds, rng) for N, E in SELF_CASES]
    record["one_query"] = one_case(1, ONE_QUERY[0], ONE_QUERY[1], False, args.rounds, rng)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
