"""GPU tests of the dynamic-range int8 simple_gru / simple_lstm (include/kws.h: kws_qmodel_create_rnn, kws_qmodel_forward;
kws_amd.quant.QuantizedRNN): the kernel against the numpy restatement (tests/int8_rnn_ref.py) -- bit for bit where the gates saturate,
within the gate-function error elsewhere --, optional outputs, the graph-captured session, accuracy after quantizing trained models,
eval.py --int8 and streaming."""
import os
import subprocess
import sys

import numpy as np
import pytest

import int8_rnn_ref
from test_quant_gpu import _task, _write_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
U = 48


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _spec(kind, C, T=30, F=20):
    from kws_amd.model import ModelSpec
    return ModelSpec(kind, C, T, F)


def _flat(spec, ws):
    p = np.zeros(spec.param_count, np.float32)
    for t, w in zip(spec.tensors, ws):
        p[t["offset"]:t["offset"] + t["size"]] = np.asarray(w, np.float32).reshape(-1)
    return p


def _features(n, seed, scale=3.0, T=30, F=20):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, T, F)) + 0.5 * rng.standard_normal((n, 1, F))).astype(np.float32)


def _linear_gru(C, seed):
    """A GRU whose gates saturate: z-gate columns with zero weights and bias -100 (z = 0 exactly), r-gate bias +100 (r = 1 exactly),
    so h' = mx_h + mh_h -- a linear recurrence entirely on the int8 path with per-step requantization.  U_h is small (spectral radius
    about 0.5) so that 30 steps stay bounded."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(-1.0, 1.3, (20, 3 * U)) * 0.3
    rk = rng.uniform(-1.0, 1.2, (U, 3 * U)) * 0.12
    b = rng.normal(0.0, 0.3, (2, 3 * U))
    k[:, :U] = 0.0
    rk[:, :U] = 0.0
    b[0, :U], b[1, :U] = -100.0, 0.0
    b[0, U:2 * U], b[1, U:2 * U] = 100.0, 0.0
    hk = rng.normal(0.0, 1.0, (U, C))
    hb = rng.normal(0.0, 0.3, C)
    return [np.asarray(w, np.float32) for w in (k, rk, b, hk, hb)]


def _random(kind, C, seed):
    """asymmetric random weights of a trained-looking scale"""
    rng = np.random.default_rng(seed)
    G = 3 if kind == "simple_gru" else 4
    k = rng.uniform(-1.0, 1.4, (20, G * U)) / np.sqrt(20) * 0.5
    rk = rng.uniform(-1.0, 1.2, (U, G * U)) / np.sqrt(U)
    b = rng.normal(0.0, 0.3, (2, G * U) if G == 3 else (G * U,))
    hk = rng.normal(0.0, 1.0, (U, C))
    hb = rng.normal(0.0, 0.3, C)
    return [np.asarray(w, np.float32) for w in (k, rk, b, hk, hb)]


@pytest.fixture(scope="module")
def linear(torch):
    from kws_amd.quant import QuantizedRNN
    C = 11
    spec = _spec("simple_gru", C)
    ws = _linear_gru(C, 3)
    q = QuantizedRNN.from_weights(spec, _flat(spec, ws))
    feat = _features(16384, 4)
    want = int8_rnn_ref.forward("simple_gru", q.arrays, feat)
    return q, feat, want


@pytest.mark.parametrize("B", [1, 17, 2047, 2048, 16384])
def test_saturated_gru_is_bit_equal_to_the_restatement(torch, linear, B):
    q, feat, (wl, wp, wa) = linear
    x = feat[-B:] if B < 16384 else feat                # B = 2047 starts at an odd clip: no alignment to the 16-clip tile
    wl, wp, wa = wl[-B:], wp[-B:], wa[-B:]
    lg, pr, am = q.forward(torch.from_numpy(x).cuda(), logits=True)
    torch.cuda.synchronize()
    lg, pr, am = lg.cpu().numpy(), pr.cpu().numpy(), am.cpu().numpy()
    assert lg.shape == (B, q.num_classes) and am.dtype == np.int32
    bad = np.nonzero((lg.view(np.uint32) != wl.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "logits differ on %d clips, first %s: %s vs %s" % (bad.size, bad[:3], lg[bad[0]], wl[bad[0]])
    np.testing.assert_allclose(pr, wp, atol=1e-6, rtol=0)
    top2 = np.sort(wl, 1)[:, -2:]
    distinct = top2[:, 1] > top2[:, 0]
    np.testing.assert_array_equal(am[distinct], wa[distinct])
    if B > 1000:                                        # not degenerate: the logits differ from clip to clip
        assert all(np.unique(wl[:, c]).size > B // 2 for c in range(q.num_classes))


@pytest.mark.parametrize("kind", ["simple_gru", "simple_lstm"])
def test_general_weights_match_the_restatement_within_the_gate_error(torch, kind):
    """With unsaturated gates the device's sigmoidf_ / tanh_fast_ differ from float64 by a few fp32 ulp (include/kws.h).  Where that
    moves no requantized code, the logits differ only through that error: the scales of h, the rescales and the head carry it, so a
    logit moves by about T (steps) x 8 ulp of its magnitude -- the tight bound below, which a majority of clips must meet (about 1500
    codes per clip, each within ~1e-4 of a tie with that probability: a flip in roughly one clip of five).  A value v * inv
    within that error of a rounding tie flips one code by one step.  That is one quantization step at one time step, where the
    quantization itself (int8 restatement against the float64 model) makes a rounding error of up to half a step on each of the ~48
    codes of every step: over T = 30 steps about sqrt(48 T) x 0.3 = 11 steps' worth.  A clip with a few flips therefore stays within
    half of the largest quantization error (0.31 of it measured for the GRU)."""
    from kws_amd.quant import QuantizedRNN
    C, T, B = 9, 30, 4096
    spec = _spec(kind, C)
    ws = _random(kind, C, 21)
    q = QuantizedRNN.from_weights(spec, _flat(spec, ws))
    feat = _features(B, 22)
    wl, _, wa = int8_rnn_ref.forward(kind, q.arrays, feat)
    lg, _, am = q.forward(torch.from_numpy(feat).cuda(), logits=True)
    lg, am = lg.cpu().numpy(), am.cpu().numpy()
    err = np.abs(lg.astype(np.float64) - wl).max(1)
    tight = T * 8 * np.finfo(np.float32).eps * (1.0 + np.abs(wl).max(1))
    clean = err <= tight
    assert clean.mean() >= 0.5, (kind, clean.mean(), np.median(err))
    qerr = np.abs(wl - int8_rnn_ref.float_forward(kind, ws, feat)).max()
    assert qerr > 0 and err.max() <= 0.5 * qerr, (kind, err.max(), qerr)
    top2 = np.sort(wl, 1)[:, -2:]
    decided = top2[:, 1] - top2[:, 0] > 2 * err.max()
    np.testing.assert_array_equal(am[decided], wa[decided])
    assert (am == wa).mean() >= 0.99


def test_optional_outputs_and_empty_batch(torch, linear):
    from kws_amd import lib as _l
    q, feat, _ = linear
    x = torch.from_numpy(feat[:40]).cuda()
    lg, pr, am = q.forward(x, logits=True)
    only = torch.full((40, q.num_classes), 7.0, device="cuda")
    q._launch(x, 40, only, None, None)
    am2 = torch.full((40,), -1, dtype=torch.int32, device="cuda")
    q._launch(x, 40, None, None, am2)
    pr2 = torch.zeros((40, q.num_classes), device="cuda")
    q._launch(x, 40, None, pr2, None)
    assert torch.equal(only, lg) and torch.equal(am2, am) and torch.equal(pr2, pr)
    p0, a0 = q.forward(torch.zeros((0, 30, 20), device="cuda"))
    assert p0.shape == (0, q.num_classes) and a0.shape == (0,)
    L = _l.get_lib()
    assert L.kws_qmodel_forward(q._handle(), None, 0, None, 0, None, None, None, None) == 0
    assert L.kws_qmodel_workspace_bytes(q._handle(), 4096) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["simple_gru", "simple_lstm"])
def test_quantized_session_graph_replay_equals_eager(torch, kind):
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from kws_amd.inference import InferenceSession
    from kws_amd.model import DeviceModel
    from kws_amd.quant import QuantizedRNN
    C, B = 7, 33
    spec = _spec(kind, C)
    ws = _random(kind, C, 5)
    dm = DeviceModel(_spec(kind, C))
    dm.set_weights(ws)
    q = QuantizedRNN.from_model(dm)
    assert np.array_equal(q.arrays["kernel"], QuantizedRNN.from_weights(spec, _flat(spec, ws)).arrays["kernel"])
    rng = np.random.default_rng(3)
    pcm = np.clip(3000.0 * rng.standard_normal((B, 16000)), -32768, 32767).astype(np.int16)
    feat = Featurizer(pr, "mel")
    sess = InferenceSession(dm, feat, B, wav_dtype=torch.int16, use_graph=True, quantized=q)
    sess.wav.copy_(torch.from_numpy(pcm))
    probs, am = sess.run()
    torch.cuda.synchronize()
    lg_g, p_g, a_g = sess.logits.clone(), probs.clone(), am.clone()
    lg, p, a = q.forward(feat(torch.from_numpy(pcm).cuda()), logits=True)
    assert torch.equal(lg_g, lg) and torch.equal(p_g, p) and torch.equal(a_g, a)
    eager = InferenceSession(dm, feat, B, wav_dtype=torch.int16, use_graph=False, quantized=q)
    eager.wav.copy_(torch.from_numpy(pcm))
    p_e, a_e = eager.run()
    assert torch.equal(p_e, p_g) and torch.equal(a_e, a_g)


@pytest.mark.parametrize("kind", ["simple_gru", "simple_lstm"])
def test_trained_model_keeps_its_accuracy_at_int8(torch, golden, kind):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    C = 5
    rng = np.random.default_rng(17)
    pcm, x, y = _task(golden, rng, 512, 128)
    m = KWSModel(kind, C, seed=5)
    m.compile(optimizer=get_optimizer("adam", 2e-3, decay_type=None), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    m.fit(x, y, batch_size=128, epochs=12, verbose=0)
    _, xt, yt = _task(golden, np.random.default_rng(23), 2000, 400)
    a32 = m.predict(xt).argmax(-1)
    acc32 = (a32 == yt).mean()
    assert (m.predict(x).argmax(-1) == y).mean() > 0.9 and acc32 > 0.9, acc32     # the fp32 model learned the task (inference mode)
    e32 = m.predict(pcm).argmax(-1)
    with pytest.raises(ValueError):
        m.quantize(x, method="max")
    qm = m.quantize()                                   # no calibration data
    assert qm.quantized.method == "dynamic"
    np.testing.assert_array_equal(qm.predict(pcm).argmax(-1), e32)          # the eight clips, raw audio in
    a8 = qm.predict_classes(xt)
    agree, acc8 = (a8 == a32).mean(), (a8 == yt).mean()
    assert agree >= 0.98, (kind, agree)
    assert acc8 >= acc32 - 0.01, (kind, acc8, acc32)
    loss8, eacc8 = qm.evaluate(xt, yt)
    assert abs(eacc8 - acc8) < 1e-9 and np.isfinite(loss8)


def test_eval_py_int8_gru_end_to_end(torch, golden, tmp_path):
    from classifier.model import get_model
    from kws_amd import quant
    classes = ["background", "right", "left"]
    data = str(tmp_path / "data")
    _write_tree(data, golden, classes)
    cpath = str(tmp_path / "classes.txt")
    with open(cpath, "w") as f:
        f.write("\n".join(classes) + "\n")
    m = get_model("simple_gru", 3)
    wpath = str(tmp_path / "w.npz")
    m.save_weights(wpath)
    base = [sys.executable, os.path.join(PKG, "eval.py"), "--model_type", "simple_gru", "--weights_path", wpath, "--dataset_path", data,
            "--classes_path", cpath]
    from classifier.data import get_dataset
    get_dataset(data, classes)                          # the feature cache exists before either run, so both print the same lines
    plain = subprocess.run(base, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert plain.returncode == 0, plain.stderr
    qpath = str(tmp_path / "q.npz")
    out = subprocess.run(base + ["--int8", "--calib_path", str(tmp_path / "missing"), "--save_quantized", qpath], capture_output=True,
                         text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr             # --calib_path is not read for the dynamic method
    assert out.stdout.startswith(plain.stdout)
    tail = out.stdout[len(plain.stdout):]
    assert "int8 (dynamic range):" in tail and "out of 12 samples" in tail and "argmax agreement" in tail and "Saved int8 model" in tail
    q = quant.load(qpath)
    assert isinstance(q, quant.QuantizedRNN) and q.method == "dynamic" and q.num_classes == 3 and q.spec.model_type == "simple_gru"


def test_quantized_gru_stream_batch_takes_its_probabilities_from_the_int8_model(torch):
    from classifier.params import pr
    from kws_amd.model import DeviceModel
    from kws_amd.quant import QuantizedRNN
    from kws_amd.stream import StreamBatch
    C = 5
    dm = DeviceModel(_spec("simple_gru", C))
    dm.set_weights(_random("simple_gru", C, 11))
    q = QuantizedRNN.from_model(dm)
    S, chunk = 6, 1024
    names = ["background", "up", "down", "left", "right"]
    sb = StreamBatch(pr, dm, S, chunk_size=chunk, class_names=names, quantized=q)
    plain = StreamBatch(pr, dm, S, chunk_size=chunk, class_names=names)
    rng = np.random.default_rng(4)
    for t in range(20):
        pcm = np.clip(rng.normal(0, 3000, (S, chunk)), -32768, 32767).astype(np.int16)
        sb.push(pcm)
        plain.push(pcm)
        if t >= 15:
            assert torch.equal(sb.mfccs, plain.mfccs)
            want, _ = q.forward(sb.mfccs.clone())
            assert torch.equal(sb.probs, want)
            assert not torch.equal(sb.probs, plain.probs)       # the float model's probabilities are not what it reports
