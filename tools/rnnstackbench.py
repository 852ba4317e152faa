"""Train-step and inference time of simple_gru / simple_lstm with 1, 2 and 3 recurrent layers at B = 2048, T = 30, F = 20, C = 36
(tools/grubench.py's shape), and of one 48-wide layer alone (a one-layer model at F = 48).  The configurations alternate inside every
round and the figure of each is the median over the rounds, so a drift of the machine lands on all of them alike; min .. max is the
run-to-run spread of this session.  --json FILE keeps the figures."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tf-keras-speech-commands_amd"))
import torch, kws_amd
from kws_amd.model import DeviceModel, ModelSpec
from kws_amd.init import init_weights

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--steps", type=int, default=40, help="timed calls per configuration and round")
ap.add_argument("--json", type=str, default=None)
args = ap.parse_args()
B, T, C = args.batch, 30, 36
configs = [(kind, L, 20) for kind in ("simple_gru", "simple_lstm") for L in (1, 2, 3)] + [("simple_gru", 1, 48), ("simple_lstm", 1, 48)]
y = torch.randint(0, C, (B,), device="cuda", dtype=torch.int32)
models = []
for kind, L, F in configs:
    spec = ModelSpec(kind, C, T, F, num_layers=L); dm = DeviceModel(spec); dm.set_weights(init_weights(spec, 0))
    models.append((dm, torch.randn((B, T, F), device="cuda")))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps): fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


def train(dm, x): return lambda i: (dm.train_fwd_bwd(x, y, dropout_seed=i + 1), dm.adam_step())
def infer(dm, x): return lambda i: dm.forward(x)


for dm, x in models:                      # warm every shape: code objects, workspaces
    for i in range(5): train(dm, x)(i); infer(dm, x)(i)
torch.cuda.synchronize()
times = {c: {"train": [], "infer": []} for c in configs}
for r in range(args.rounds):
    for c, (dm, x) in zip(configs, models):
        times[c]["train"].append(timed(train(dm, x)))
        times[c]["infer"].append(timed(infer(dm, x)))
out = []
for c in configs:
    row = {"kind": c[0], "num_layers": c[1], "F": c[2], "B": B}
    for what in ("train", "infer"):
        v = times[c][what]
        row[what + "_ms"] = statistics.median(v); row[what + "_min_ms"] = min(v); row[what + "_max_ms"] = max(v)
    out.append(row)
    print("%-11s layers=%d F=%2d  train %.4f ms (%.4f .. %.4f)  %.2f Mclips/s   infer %.4f ms (%.4f .. %.4f)" % (
        c[0], c[1], c[2], row["train_ms"], row["train_min_ms"], row["train_max_ms"], B / row["train_ms"] / 1e3, row["infer_ms"],
        row["infer_min_ms"], row["infer_max_ms"]))
by = {(r["kind"], r["num_layers"], r["F"]): r for r in out}
for kind in ("simple_gru", "simple_lstm"):
    for what in ("train", "infer"):
        one, two, three, alone = [by[(kind, L, 20)][what + "_ms"] for L in (1, 2, 3)] + [by[(kind, 1, 48)][what + "_ms"]]
        print("%-11s %-5s per added layer: +%.4f ms (1 -> 2), +%.4f ms (2 -> 3); one F = 48 layer with its head alone: %.4f ms" % (
            kind, what, two - one, three - two, alone))
kws_amd.lib.prof_enable(True)
for c, (dm, x) in zip(configs, models):
    if c[1] != 3: continue
    for i in range(10): train(dm, x)(i)
    torch.cuda.synchronize()
    rep = kws_amd.lib.prof_report()
    print(c[0], "3 layers, per launch name (ms per step, the three layers summed):")
    for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])[:4]: print("  %-28s %.4f ms" % (k, v["total_ms"] / 10))
    kws_amd.lib.prof_enable(False); kws_amd.lib.prof_enable(True)
if args.json:
    with open(args.json, "w") as f: json.dump({"build_id": kws_amd.lib.build_id(), "rows": out}, f, indent=1)
