"""The head bank in figures (kws_heads_apply, kws_amd.transfer.HeadBank), at E = 128, C = 12:

  serving     R = 16384 rows, every row a head of its own (a bank of 16384 heads, 101 MB): the kernel's own time (the library's
              per-launch timing), and the same product from torch operators (baddbmm over the gathered weights, softmax);
  one head    R = 16384 rows of ONE head: every tile is a run and reads the head from LDS;
  no runs     the same rows and the same weights under two head ids that alternate, so that no tile is a run and every row reads
              its head from memory (L2): the difference to `one head` is what the LDS run route buys;
  folds       R = 1M rows in 64 runs of 16384 (the score_heads shape), with runs and -- aliased ids again -- without, against the
              loop of torch matrix products cross_validate scores its folds with (float64, as there);
  push        StreamServer.push at S = 4096 slots, every slot pushed, 1024 samples each: without a bank (the fused forward, the
              path every commit before the bank had) and with a bank of 512 heads (kws_model_embed + kws_heads_apply).

  discrepancy the bank's probabilities against the model's own forward with the same head (what with_head builds), four model kinds.

The tool reports, it asserts no ratio.

    python tools/headbankbench.py [--rounds 9] [--out profiles/headbankbench.json]

Every figure is the median of --rounds repetitions after warm-up runs of the same work (min and max kept); the variants of one
comparison alternate.  The last line printed is the record as one JSON line."""
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

E, C = 128, 12
R_SERVE, RUNS, R_FOLDS = 16384, 64, 1 << 20
HEAD_BYTES = 4 * (E + 1) * C


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_ms(fn, name="heads_apply_kernel"):
    _l.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    rep = _l.prof_report()
    _l.prof_enable(False)
    return rep[name]["total_ms"]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def alternate(rounds, **variants):
    """-> {name: [ms]}: one repetition of every variant per round, after two warm-up rounds"""
    out = {k: [] for k in variants}
    for i in range(rounds + 2):
        for k, fn in variants.items():
            v = fn()
            if i >= 2:
                out[k].append(v)
    return out


def random_heads(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.2, 0.2, (n, E, C)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, C)).astype(np.float32))


def fill(bank, kernels, biases, at=0):
    """heads into consecutive slots in one copy (every slot has room for max_classes = C classes)"""
    room = int(bank.offsets[1] - bank.offsets[0]) if bank.capacity > 1 else bank.count
    n = kernels.shape[0]
    flat = np.zeros((n, room), np.float32)
    flat[:, :E * C] = kernels.reshape(n, -1)
    flat[:, E * C:(E + 1) * C] = biases
    bank.weights[at * room:(at + n) * room].copy_(torch.from_numpy(flat.reshape(-1)))
    bank.head_classes[at:at + n].fill_(C)
    bank.classes[at:at + n] = C


def serving(rounds):
    k, b = random_heads(R_SERVE, 0)
    bank = T.HeadBank(E, R_SERVE, C)
    fill(bank, k, b)
    emb = torch.randn((R_SERVE, E), device="cuda")
    ids = torch.randperm(R_SERVE, device="cuda").to(torch.int32)
    W, B = torch.from_numpy(k).cuda(), torch.from_numpy(b).cuda()
    idl = ids.long()

    def torch_way():
        return torch.softmax(torch.baddbmm(B.index_select(0, idl)[:, None, :], emb[:, None, :], W.index_select(0, idl))[:, 0, :], 1)

    probs = bank.launch(emb, R_SERVE, ids, want=("probs",))[0]
    diff = float((probs - torch_way()).abs().max())
    t = alternate(rounds, kernel=lambda: kernel_ms(lambda: bank.launch(emb, R_SERVE, ids, want=("probs",))),
                  call=lambda: event_ms(lambda: bank.launch(emb, R_SERVE, ids, want=("probs",))), torch=lambda: event_ms(torch_way))
    bytes_row = HEAD_BYTES + 4 * E + 4 * C + 4
    rec = {"rows": R_SERVE, "heads": R_SERVE, "kernel_ms": med(t["kernel"]), "call_ms": med(t["call"]), "torch_baddbmm_ms": med(t["torch"]),
           "bytes_per_row": bytes_row, "kernel_TBps": bytes_row * R_SERVE / (statistics.median(t["kernel"]) * 1e-3) / 1e12,
           "max_abs_probability_difference_to_torch": diff}
    print("serving   %d rows, a head each: kernel %.4f ms (%.2f TB/s of %d B per row), call %.4f ms, torch baddbmm %.4f ms; differ by %.2g"
          % (R_SERVE, rec["kernel_ms"]["median"], rec["kernel_TBps"], bytes_row, rec["call_ms"]["median"], rec["torch_baddbmm_ms"]["median"], diff),
          flush=True)
    return rec


def runs_case(name, R, n_runs, rounds, torch_loop):
    """R rows in n_runs runs of one head each: with the run route, and with every head under two alternating ids (no tile is a run)"""
    k, b = random_heads(n_runs, 1)
    bank = T.HeadBank(E, 2 * n_runs, C)
    fill(bank, k, b)
    fill(bank, k, b, at=n_runs)                                   # slot n_runs + h holds head h's weights again
    emb = torch.randn((R, E), device="cuda")
    per = R // n_runs
    run_ids = torch.arange(n_runs, dtype=torch.int32, device="cuda").repeat_interleave(per)
    alias_ids = run_ids + n_runs * (torch.arange(R, dtype=torch.int32, device="cuda") & 1)
    a = bank.launch(emb, R, run_ids, want=("probs", "pred"))
    c = bank.launch(emb, R, alias_ids, want=("probs", "pred"))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])   # the two routes: the same bits
    variants = dict(runs=lambda: kernel_ms(lambda: bank.launch(emb, R, run_ids, want=("probs", "pred"))),
                    no_runs=lambda: kernel_ms(lambda: bank.launch(emb, R, alias_ids, want=("probs", "pred"))))
    if torch_loop:
        y = torch.randint(0, C, (R,), device="cuda")
        W, B = torch.from_numpy(k).cuda(), torch.from_numpy(b).cuda()
        rows = [torch.arange(h * per, (h + 1) * per, device="cuda") for h in range(n_runs)]

        def loop():                                              # cross_validate's scoring, fold after fold
            for h in range(n_runs):
                logits = emb.index_select(0, rows[h]).double() @ W[h].double() + B[h].double()
                yt = y.index_select(0, rows[h])
                (logits.argmax(1) == yt).double().mean()
                torch.nn.functional.cross_entropy(logits, yt)

        variants["torch"] = lambda: event_ms(loop)
    t = alternate(rounds, **variants)
    bytes_row = 4 * E + 4 * C + 8                                 # the embedding in, probabilities and pred out; the head is shared
    rec = {"rows": R, "runs": n_runs, "runs_ms": med(t["runs"]), "no_runs_ms": med(t["no_runs"]), "bytes_per_row": bytes_row,
           "runs_TBps": bytes_row * R / (statistics.median(t["runs"]) * 1e-3) / 1e12}
    line = "%-9s %d rows in %d runs: run route %.4f ms (%.2f TB/s of %d B per row), the same without runs %.4f ms" \
        % (name, R, n_runs, rec["runs_ms"]["median"], rec["runs_TBps"], bytes_row, rec["no_runs_ms"]["median"])
    if torch_loop:
        rec["torch_loop_ms"] = med(t["torch"])
        line += ", torch loop (float64) %.3f ms" % rec["torch_loop_ms"]["median"]
    print(line, flush=True)
    return rec


def push_case(rounds, S=4096, n_heads=512):
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    from kws_amd.stream import StreamServer
    spec = ModelSpec("simple_cnn", C, pr.n_features, pr.n_mfcc)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, seed=0))
    k, b = random_heads(n_heads, 2)
    bank = T.HeadBank(E, n_heads, C)
    fill(bank, k, b)
    plain = StreamServer(pr, dm, S)
    banked = StreamServer(pr, dm, S, heads=bank)
    rng = np.random.default_rng(3)
    slots = [plain.open() for _ in range(S)]
    assert [banked.open(head=int(h)) for h in rng.integers(0, n_heads, S)] == slots
    pcm = torch.from_numpy(np.clip(rng.normal(0, 3000, (S, 1024)), -32768, 32767).astype(np.int16)).cuda()
    t = alternate(rounds, plain=lambda: wall_ms(lambda: plain.push(slots, pcm)), bank=lambda: wall_ms(lambda: banked.push(slots, pcm)),
                  embed=lambda: event_ms(lambda: dm.embed(banked._feat)), forward=lambda: event_ms(lambda: dm.forward(banked._feat, True, False)))
    rec = {"slots": S, "heads": n_heads, "chunk": 1024, "model": "simple_cnn", "plain_push_ms": med(t["plain"]), "bank_push_ms": med(t["bank"]),
           "embed_ms": med(t["embed"]), "fused_forward_ms": med(t["forward"])}
    print("push      S = %d: plain %.3f ms, with a bank of %d heads %.3f ms (of it: kws_model_embed %.3f ms against the fused forward's %.3f ms)"
          % (S, rec["plain_push_ms"]["median"], n_heads, rec["bank_push_ms"]["median"], rec["embed_ms"]["median"],
             rec["fused_forward_ms"]["median"]), flush=True)
    return rec


def discrepancy(B=4096):
    """the bank's probabilities against the model's own forward with the same head behind the same backbone (what with_head builds):
    the fused forwards never materialise the embedding, so the two need not agree to the bit"""
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    out = []
    feat = torch.randn((B, pr.n_features, pr.n_mfcc), device="cuda")
    for kind in ("simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"):
        spec = ModelSpec(kind, C, pr.n_features, pr.n_mfcc)
        dm = DeviceModel(spec)
        w = init_weights(spec, seed=1)
        dm.set_weights(w)
        bank = T.HeadBank.from_fits([(w[-2], w[-1])])
        own = dm.forward(feat, True, False)[0]
        emb = dm.embed(feat)
        got = bank.launch(emb, B, torch.zeros(B, dtype=torch.int32, device="cuda"), want=("probs",))[0]
        d = (own - got).abs()
        out.append({"model": kind, "clips": B, "max_abs_difference": float(d.max()), "rows_not_bit_identical": int((own != got).any(1).sum())})
        print("discrepancy %-16s bank against the model's forward: max |dp| %.3g, %d of %d rows differ in some bit"
              % (kind, out[-1]["max_abs_difference"], out[-1]["rows_not_bit_identical"], B), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "E": E, "C": C,
              "conditions": "two warm-up rounds of the same work first, then the median of `rounds` repetitions (min and max kept); the "
                            "variants of a comparison alternate; kernel times are the library's per-launch timing, torch and push times "
                            "events / wall clock around the call with a synchronisation",
              "build_id": {k: _l.build_id().get(k) for k in ("kws_heads.hip", "kws_model.hip", "kws_stream.hip")}}
    record["serving"] = serving(args.rounds)
    record["one_head"] = runs_case("one head", R_SERVE, 1, args.rounds, torch_loop=False)
    record["folds"] = runs_case("folds", R_FOLDS, RUNS, args.rounds, torch_loop=True)
    record["push"] = push_case(args.rounds)
    record["discrepancy_to_own_forward"] = discrepancy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
