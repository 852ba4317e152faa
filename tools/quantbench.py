"""Cost of the int8 simple_cnn (kws_amd.quant) at B = 4096 against the fp32-level forward it replaces: the forward alone (features in,
probabilities out; fp32 = kws_model_forward with its weight tables prepared, int8 = kws_qmodel_forward) and the graph-captured
featurize + forward of kws_amd.inference.InferenceSession for each.  Variants alternate within each round (several rounds, medians).
Next to every time stand the algorithmic bytes and int8 ops and the HBM, matrix and VALU floors.  Kernel-only times for DESIGN.md come
from a separate `rocprofv3 --kernel-trace --stats` run of `--kernel-only`.  Prints one JSON line; --out also writes it to a file.

    python tools/quantbench.py [--rounds 7] [--out quantbench.json] [--kernel-only]

--model simple_cnn_lite: the int8 simple_cnn_lite forward against the fp32 and the fp16 lite forwards (kws_model_forward at
KWS_INFER_FP32 / KWS_INFER_FP16, weight tables prepared) and the three graph-captured featurize + forward sessions, at B = 4096 and
16 384 (--batches).

--model simple_gru / simple_lstm: the dynamic-range int8 forward (kws_qmodel_forward on a kws_qmodel_create_rnn handle) against the fp32
recurrent forward + head (kws_model_forward), and the two graph-captured featurize + forward sessions, at B = 2048 and 16 384.

--calib kl: the calibration passes of the KL method for both models at B = 4096 (--calib-batch): the max pass (kws_model_calibrate[_lite])
and the histogram pass (kws_model_calibrate_hist) alternating within each round, then the KL search on the host (kws_quant_kl_ranges)
over the histograms of that set.  With --kernel-only it only launches the two passes of both models."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_GBS = 6300.0          # MI355X HBM3E, measured copy bandwidth
I8_TOPS = 5000.0          # dense int8 matrix peak (v_mfma_i32_16x16x64_i8)
VALU_TOPS = 78.6          # 32-bit vector ops per second (256 CUs x 128 lanes x 2.4 GHz), one op per lane and cycle

# int8 multiply-adds per clip of the forward: conv1 on the vector ALU, the rest on the matrix cores
MACS_VALU = 600 * 16 * 9
MACS_MATRIX = 150 * 32 * 144 + 12 * 64 * 288 + 12 * 128 * 576 + 256 * 128 + 128 * 36
# simple_cnn_lite, as the kernel computes it (only the pixels pooling keeps): depthwise 1..4 and pointwise 1 on the vector ALU,
# pointwise 2..4, Dense and head on the matrix cores
LITE_MACS_VALU = 600 * 9 + 600 * 16 + 140 * 16 * 9 + 12 * 32 * 9 + 8 * 64 * 9
LITE_MACS_MATRIX = 140 * 16 * 32 + 12 * 32 * 64 + 8 * 64 * 128 + 256 * 128 + 128 * 36


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


def floors(B, C, macs_matrix=MACS_MATRIX, macs_valu=MACS_VALU, macs_per_valu_op=4):
    """bytes (features in, probabilities and arg-max out), int8 ops and the three floors (ms) of one int8 forward"""
    nbytes = B * (600 * 4 + C * 4 + 4)
    ops_m, ops_v = 2 * B * macs_matrix, 2 * B * macs_valu
    return {"bytes": int(nbytes), "int8_matrix_ops": int(ops_m), "int8_valu_ops": int(ops_v),
            "hbm_floor_ms": round(nbytes / (HBM_GBS * 1e6), 5), "matrix_floor_ms": round(ops_m / (I8_TOPS * 1e9), 5),
            "valu_floor_ms": round(B * macs_valu / macs_per_valu_op / (VALU_TOPS * 1e9), 5)}   # simple_cnn: v_dot4, four per op


def lite_main(args):
    """--model simple_cnn_lite: fp32 / fp16 / int8 forwards and graph-captured sessions, alternating within each round"""
    from classifier.params import pr
    from kws_amd import lib as _l
    from kws_amd.featurizer import Featurizer
    from kws_amd.inference import InferenceSession
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    from kws_amd.quant import QuantizedCNNLite, calibrate
    torch.manual_seed(0)
    C = 36
    spec = ModelSpec("simple_cnn_lite", C, pr.n_features, pr.feature_size)
    w = init_weights(spec, seed=0)
    # one ModelSpec each: the precision attribute belongs to the library's model handle, which a ModelSpec owns
    dm = {n: DeviceModel(ModelSpec("simple_cnn_lite", C, pr.n_features, pr.feature_size)) for n in ("fp32", "fp16")}
    for m in dm.values():
        m.set_weights(w)
    dm["fp32"].set_precision(infer=_l.INFER_FP32)
    dm["fp16"].set_precision(infer=_l.INFER_FP16)
    fz = Featurizer(pr)
    out = {"model": "simple_cnn_lite", "C": C, "runs": []}
    for B in args.batches:
        feat = (3.0 * torch.randn((B, pr.n_features, pr.feature_size), device="cuda")).contiguous()
        q = QuantizedCNNLite.from_model(dm["fp32"], calibrate(dm["fp32"], feat[:4096]), "max")
        ws = {n: m.new_workspace(B) for n, m in dm.items()}
        for n, m in dm.items():
            m.prepare_inference(B, workspace=ws[n])
        probs = torch.empty((B, C), device="cuda")
        am = torch.empty((B,), dtype=torch.int32, device="cuda")
        fwd = {"fp32": lambda: dm["fp32"].forward(feat, workspace=ws["fp32"]), "fp16": lambda: dm["fp16"].forward(feat, workspace=ws["fp16"]),
               "int8": lambda: q._launch(feat, B, None, probs, am)}
        if args.kernel_only:
            for _ in range(args.iters):
                for f in fwd.values():
                    f()
            torch.cuda.synchronize()
            out["runs"].append({"B": B, "kernel_only": True, "launches": len(fwd) * args.iters})
            continue
        sess = {"fp32": InferenceSession(dm["fp32"], fz, B, wav_dtype=torch.int16),
                "fp16": InferenceSession(dm["fp32"], fz, B, wav_dtype=torch.int16, fp16=True),
                "int8": InferenceSession(dm["fp32"], fz, B, wav_dtype=torch.int16, quantized=q)}
        pcm = torch.randint(-3000, 3000, (B, pr.max_samples), dtype=torch.int16, device="cuda")
        for s in sess.values():
            s.wav.copy_(pcm)
        res = {"B": B, "int8_floors": floors(B, C, LITE_MACS_MATRIX, LITE_MACS_VALU, 1), "forward": {}, "featurize_forward_graph": {}}
        ft = {n: [] for n in fwd}
        gt = {n: [] for n in sess}
        for _ in range(args.rounds):
            for n, f in fwd.items():
                ft[n].append(time_ms(f, args.iters))
            for n, s in sess.items():
                gt[n].append(time_ms(s.run, args.iters))
        for n in fwd:
            res["forward"][n] = {"median_ms": round(float(np.median(ft[n])), 4), "rounds": [round(x, 4) for x in ft[n]]}
            res["featurize_forward_graph"][n] = {"median_ms": round(float(np.median(gt[n])), 4), "rounds": [round(x, 4) for x in gt[n]]}
        res["fp32_int8_argmax_agreement_random_weights"] = round(float((sess["fp32"].argmax == sess["int8"].argmax).float().mean().item()), 4)
        out["runs"].append(res)
        del sess, ws
    out["device"] = torch.cuda.get_device_name(0)
    return out


def rnn_floors(B, C, G, T=30, F=20):
    """bytes (features in, probabilities and arg-max out), int8 matrix ops (the padded k-steps the kernel issues: K = 64 for x_t W and
    h U, 3 G column tiles each, per step; the head's three tiles) and the VALU floor of the gate arithmetic (about 20 fp32 ops per
    gate value and step, counted from the kernel's source) of one dynamic-range int8 forward"""
    nbytes = B * (T * F * 4 + C * 4 + 4)
    ops_m = 2 * B * (T * 2 * 64 * 48 * G + 64 * 48)
    ops_v = B * T * 48 * G * 20
    return {"bytes": int(nbytes), "int8_matrix_ops": int(ops_m), "valu_ops": int(ops_v),
            "hbm_floor_ms": round(nbytes / (HBM_GBS * 1e6), 5), "matrix_floor_ms": round(ops_m / (I8_TOPS * 1e9), 5),
            "valu_floor_ms": round(ops_v / (VALU_TOPS * 1e9), 5)}


def rnn_main(args):
    """--model simple_gru / simple_lstm: the fp32 recurrent forward + head (kws_model_forward) against the dynamic-range int8 kernel,
    and the two graph-captured featurize + forward sessions, alternating within each round"""
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from kws_amd.inference import InferenceSession
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    from kws_amd.quant import QuantizedRNN
    torch.manual_seed(0)
    C, G = 36, 3 if args.model == "simple_gru" else 4
    spec = ModelSpec(args.model, C, pr.n_features, pr.feature_size)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, seed=0))
    q = QuantizedRNN.from_model(dm)
    fz = Featurizer(pr)
    out = {"model": args.model, "C": C, "runs": []}
    for B in args.batches:
        feat = (3.0 * torch.randn((B, pr.n_features, pr.feature_size), device="cuda")).contiguous()
        ws = dm.new_workspace(B)
        dm.prepare_inference(B, workspace=ws)
        probs = torch.empty((B, C), device="cuda")
        am = torch.empty((B,), dtype=torch.int32, device="cuda")
        fwd = {"fp32": lambda: dm.forward(feat, workspace=ws), "int8": lambda: q._launch(feat, B, None, probs, am)}
        if args.kernel_only:
            for _ in range(args.iters):
                for f in fwd.values():
                    f()
            torch.cuda.synchronize()
            out["runs"].append({"B": B, "kernel_only": True, "launches": len(fwd) * args.iters})
            continue
        sess = {"fp32": InferenceSession(dm, fz, B, wav_dtype=torch.int16),
                "int8": InferenceSession(dm, fz, B, wav_dtype=torch.int16, quantized=q)}
        pcm = torch.randint(-3000, 3000, (B, pr.max_samples), dtype=torch.int16, device="cuda")
        for s in sess.values():
            s.wav.copy_(pcm)
        res = {"B": B, "int8_floors": rnn_floors(B, C, G, pr.n_features, pr.feature_size), "forward": {}, "featurize_forward_graph": {}}
        ft = {n: [] for n in fwd}
        gt = {n: [] for n in sess}
        for _ in range(args.rounds):
            for n, f in fwd.items():
                ft[n].append(time_ms(f, args.iters))
            for n, s in sess.items():
                gt[n].append(time_ms(s.run, args.iters))
        for n in fwd:
            res["forward"][n] = {"median_ms": round(float(np.median(ft[n])), 4), "rounds": [round(x, 4) for x in ft[n]]}
            res["featurize_forward_graph"][n] = {"median_ms": round(float(np.median(gt[n])), 4), "rounds": [round(x, 4) for x in gt[n]]}
        res["fp32_int8_argmax_agreement_random_weights"] = round(float((sess["fp32"].argmax == sess["int8"].argmax).float().mean().item()), 4)
        out["runs"].append(res)
        del sess, ws
    out["device"] = torch.cuda.get_device_name(0)
    return out


def calib_main(args):
    """--calib kl: max pass, histogram pass and host KL search for simple_cnn and simple_cnn_lite"""
    import time
    from classifier.params import pr
    from kws_amd import lib as _l
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    from kws_amd.quant import calibrate, histograms
    torch.manual_seed(0)
    B, C = args.calib_batch, 36
    feat = (3.0 * torch.randn((B, pr.n_features, pr.feature_size), device="cuda")).contiguous()
    L = _l.get_lib()
    out = {"calib": "kl", "B": B, "C": C, "models": {}}
    for model in ("simple_cnn", "simple_cnn_lite"):
        spec = ModelSpec(model, C, pr.n_features, pr.feature_size)
        dm = DeviceModel(spec)
        dm.set_weights(init_weights(spec, seed=0))
        amax = calibrate(dm, feat)
        T = amax.size
        amax_d = torch.zeros((T,), dtype=torch.float32, device="cuda")
        hist = torch.zeros((T, _l.QUANT_HIST_BINS), dtype=torch.int64, device="cuda")
        passes = {"max": lambda: calibrate(dm, feat, amax=amax_d), "hist": lambda: histograms(dm, feat, amax, hist=hist)}
        if args.kernel_only:
            for _ in range(args.iters):
                for f in passes.values():
                    f()
            torch.cuda.synchronize()
            out["models"][model] = {"kernel_only": True, "launches": len(passes) * args.iters}
            continue
        # calibrate() copies its maxima to the host after the launch; time the launches alone
        fmax = lambda: _l.check(getattr(L, "kws_model_calibrate_lite" if model == "simple_cnn_lite" else "kws_model_calibrate")(
            spec.handle, feat.data_ptr(), B, dm.params.data_ptr(), dm.state.data_ptr(), None, 0, amax_d.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
        passes["max"] = fmax
        t = {n: [] for n in passes}
        for _ in range(args.rounds):
            for n, f in passes.items():
                t[n].append(time_ms(f, args.iters))
        hist.zero_()
        histograms(dm, feat, amax, hist=hist)
        h = np.ascontiguousarray(hist.cpu().numpy().astype(np.uint64))
        ranges, bins = np.zeros(T, np.float32), np.zeros(T, np.int32)
        ks = []
        for _ in range(3):
            t0 = time.perf_counter()
            _l.check(L.kws_quant_kl_ranges(h.ctypes.data, amax.ctypes.data, T, ranges.ctypes.data, bins.ctypes.data))
            ks.append(time.perf_counter() - t0)
        res = {"T": T, "pass_ms": {n: {"median_ms": round(float(np.median(v)), 4), "rounds": [round(x, 4) for x in v]} for n, v in t.items()},
               "kl_search_host_s": round(float(np.median(ks)), 4), "amax": [round(float(v), 4) for v in amax],
               "kl_ranges": [round(float(v), 4) for v in ranges], "kl_bins": bins.tolist()}
        res["hist_over_max"] = round(res["pass_ms"]["hist"]["median_ms"] / res["pass_ms"]["max"]["median_ms"], 3)
        out["models"][model] = res
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true", help="only launch the two forwards (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="simple_cnn", choices=["simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"])
    ap.add_argument("--batches", type=int, nargs="+", default=None,
                    help="simple_cnn_lite (default 4096 16384), simple_gru / simple_lstm (default 2048 16384): the batch sizes")
    ap.add_argument("--calib", default=None, choices=["kl"], help="time the calibration passes of the KL method instead of the forwards")
    ap.add_argument("--calib-batch", type=int, default=4096)
    args = ap.parse_args()
    rnn = args.model in ("simple_gru", "simple_lstm")
    if args.batches is None:
        args.batches = [2048, 16384] if rnn else [4096, 16384]
    if args.calib or args.model != "simple_cnn":
        res = calib_main(args) if args.calib else rnn_main(args) if rnn else lite_main(args)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from kws_amd.inference import InferenceSession
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    from kws_amd.quant import QuantizedCNN, calibrate
    torch.manual_seed(0)
    B, C = 4096, 36
    spec = ModelSpec("simple_cnn", C, pr.n_features, pr.feature_size)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, seed=0))
    feat = (3.0 * torch.randn((B, pr.n_features, pr.feature_size), device="cuda")).contiguous()
    q = QuantizedCNN.from_model(dm, calibrate(dm, feat), "max")
    ws = dm.new_workspace(B)
    dm.prepare_inference(B, workspace=ws)
    probs = torch.empty((B, C), device="cuda")
    am = torch.empty((B,), dtype=torch.int32, device="cuda")
    fwd = {"fp32": lambda: dm.forward(feat, workspace=ws), "int8": lambda: q._launch(feat, B, None, probs, am)}
    if args.kernel_only:
        for _ in range(args.iters):
            for f in fwd.values():
                f()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": len(fwd) * args.iters}))
        return

    fz = Featurizer(pr)
    sess = {"fp32": InferenceSession(dm, fz, B, wav_dtype=torch.int16), "int8": InferenceSession(dm, fz, B, wav_dtype=torch.int16, quantized=q)}
    pcm = torch.randint(-3000, 3000, (B, pr.max_samples), dtype=torch.int16, device="cuda")
    for s in sess.values():
        s.wav.copy_(pcm)
    res = {"B": B, "C": C, "int8_floors": floors(B, C), "forward": {}, "featurize_forward_graph": {}}
    ft = {n: [] for n in fwd}
    gt = {n: [] for n in sess}
    for _ in range(args.rounds):
        for n, f in fwd.items():
            ft[n].append(time_ms(f, args.iters))
        for n, s in sess.items():
            gt[n].append(time_ms(s.run, args.iters))
    for n in fwd:
        res["forward"][n] = {"median_ms": round(float(np.median(ft[n])), 4), "rounds": [round(x, 4) for x in ft[n]]}
        res["featurize_forward_graph"][n] = {"median_ms": round(float(np.median(gt[n])), 4), "rounds": [round(x, 4) for x in gt[n]]}
    agree = float((sess["fp32"].argmax == sess["int8"].argmax).float().mean().item())
    res["fp32_int8_argmax_agreement_random_weights"] = round(agree, 4)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
