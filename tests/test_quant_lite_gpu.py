"""GPU tests of the int8 simple_cnn_lite (include/kws.h: kws_model_calibrate_lite, kws_qmodel_create_lite, kws_qmodel_forward;
kws_amd.quant.QuantizedCNNLite): calibration against the float64 oracle, the int8 kernel bit for bit against the numpy integer
restatement (tests/int8_lite_ref.py), the graph-captured session, accuracy after quantizing a trained model, eval.py --int8 and the
quantized StreamBatch."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import int8_lite_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
SEP = (0, 4, 8, 11)                                   # the SeparableConv2D layers of the oracle model


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _weights(C, seed, shift=0.25, head_gain=1.0):
    """oracle glorot weights made asymmetric (`shift`), with non-trivial BatchNorm statistics, pointwise biases and one negative gamma;
    `head_gain` scales the head kernel (an untrained net otherwise answers one class for every clip)"""
    from oracle import model_oracle as mo
    om = mo.Model("simple_cnn_lite", C).init_weights(seed)
    rng = np.random.default_rng(seed + 100)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n.endswith("kernel"):
            ws[i] = ws[i] * 1.3 + shift * np.abs(ws[i]).mean()
        elif n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.2 * rng.standard_normal(ws[i].shape)
    ws[10][2] = -0.7                                    # batch_normalization_1/gamma[2] < 0
    ws[-2] = (ws[-2] - ws[-2].mean(0)) * head_gain      # zero column sums: the shared positive mean of d decides nothing
    om.set_weights([np.asarray(w, np.float32).astype(np.float64) for w in ws])     # the device's float32 weights, exactly
    return om


def _device_model(om, C):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec("simple_cnn_lite", C, 30, 20))
    dm.set_weights([w.astype(np.float32) for w in om.get_weights()])
    return dm


def _features(n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, 30, 20)) + 0.5 * rng.standard_normal((n, 1, 20))).astype(np.float32)


def _oracle_maxima(om, feat):
    x = feat.astype(np.float64)[..., None]
    out = [np.abs(x).max()]
    for i, l in enumerate(om.layers[:-1]):
        x = l.forward(x, False)
        if i in SEP:
            out.append(np.abs(l.cache[2]).max())         # u_l: the depthwise output
        if i in (3, 7, 10, 14, 18):                      # pool 1, pool 2, stage 3's ReLU6, pool 4, Dense's ReLU6
            out.append(x.max())
    return np.array(out)


def test_calibration_matches_the_oracle_and_folds_batches(torch):
    from kws_amd.quant import calibrate
    C = 7
    om = _weights(C, 1, shift=0.0)
    dm = _device_model(om, C)
    feat = _features(300, 2, scale=0.3)
    want = _oracle_maxima(om, feat)
    got = calibrate(dm, torch.from_numpy(feat).cuda())
    assert got.shape == (10,) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    assert (want[[2, 4, 6, 8, 9]] < 6).all()             # no activation is saturated: the comparison says something
    amax = torch.zeros((10,), dtype=torch.float32, device="cuda")
    calibrate(dm, feat[:137], amax=amax)
    halves = calibrate(dm, feat[137:], amax=amax)
    assert np.array_equal(halves, got)
    assert np.array_equal(calibrate(dm, [feat[:50], feat[50:]]), got)
    assert np.array_equal(calibrate(dm, feat[:0]), np.zeros(10, np.float32))


@pytest.fixture(scope="module")
def qsetup(torch):
    from kws_amd.quant import QuantizedCNNLite, calibrate
    C = 11
    om = _weights(C, 7, shift=0.05, head_gain=4.0)
    feat = _features(16384, 8, scale=3.0)
    x = feat[:512].astype(np.float64)[..., None]
    for l in om.layers[:-1]:
        x = l.forward(x, False)
    ws = om.get_weights()
    ws[-1] = -(x.mean(0) @ ws[-2])                      # centred head: every class wins somewhere (an arg-max check that says something)
    om.set_weights(ws)
    dm = _device_model(om, C)
    amax = calibrate(dm, feat[:1024])
    q = QuantizedCNNLite.from_model(dm, amax, "max")
    outs = [int8_lite_ref.forward(q.arrays, feat[i:i + 1024]) for i in range(0, len(feat), 1024)]
    ref = tuple(np.concatenate([o[k] for o in outs]) for k in range(3))     # clips are independent: slices of it are references
    return dm, q, feat, ref


@pytest.mark.parametrize("B", [1, 17, 4095, 4096, 16384])
def test_int8_lite_forward_is_bit_equal_to_the_integer_restatement(torch, qsetup, B):
    dm, q, feat, ref = qsetup
    x = feat[-B:]                                        # B = 4095 starts at an odd clip: no alignment to the clip group
    lg, pr, am = q.forward(torch.from_numpy(x).cuda(), logits=True)
    torch.cuda.synchronize()
    lg, pr, am = lg.cpu().numpy(), pr.cpu().numpy(), am.cpu().numpy()
    wl, wp, wa = (r[-B:] for r in ref)
    assert lg.shape == (B, q.num_classes) and am.dtype == np.int32
    bad = np.nonzero((lg.view(np.uint32) != wl.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "logits differ on %d clips, first %s: %s vs %s" % (bad.size, bad[:3], lg[bad[0]], wl[bad[0]])
    np.testing.assert_allclose(pr, wp, atol=1e-6, rtol=0)
    top2 = np.sort(wl, 1)[:, -2:]
    distinct = top2[:, 1] > top2[:, 0]
    np.testing.assert_array_equal(am[distinct], wa[distinct])
    if B > 1000:                                         # the logits are not degenerate: they differ from clip to clip
        assert all(np.unique(wl[:, c]).size > 1000 for c in range(q.num_classes))
        assert np.unique(wa).size >= q.num_classes - 2


def test_int8_lite_forward_optional_outputs_and_empty_batch(torch, qsetup):
    from kws_amd import lib as _l
    dm, q, feat, _ = qsetup
    x = torch.from_numpy(feat[:40]).cuda()
    lg, pr, am = q.forward(x, logits=True)
    only = torch.full((40, q.num_classes), 7.0, device="cuda")
    q._launch(x, 40, only, None, None)
    am2 = torch.full((40,), -1, dtype=torch.int32, device="cuda")
    q._launch(x, 40, None, None, am2)
    pr2 = torch.full((40, q.num_classes), -1.0, device="cuda")
    q._launch(x, 40, None, pr2, None)
    assert torch.equal(only, lg) and torch.equal(am2, am) and torch.equal(pr2, pr)
    p0, a0 = q.forward(torch.zeros((0, 30, 20), device="cuda"))
    assert p0.shape == (0, q.num_classes) and a0.shape == (0,)
    L = _l.get_lib()
    assert L.kws_qmodel_forward(q._handle(), None, 0, None, 0, None, None, None, None) == 0
    assert L.kws_qmodel_workspace_bytes(q._handle(), 4096) == 0
    torch.cuda.synchronize()


def test_quantized_lite_session_graph_replay_equals_eager(torch, qsetup):
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from kws_amd.inference import InferenceSession
    dm, q, _, _ = qsetup
    B = 33
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


def _task(golden, rng, n, bg):
    """the separable task of tests/test_quant_gpu.py: noisy copies of the eight example clips' features (labels 1..4) plus quiet
    background (class 0)"""
    from oracle import featurizer_oracle as fo
    names = ["right_1", "left_1", "up_1", "down_1", "right_2", "left_2", "up_2", "down_2"]
    pcm = np.stack([golden["pcm_" + k] for k in names])
    feats = fo.featurize_batch(pcm.astype(np.float32) / 32768.0).astype(np.float64)
    lab = np.array([1, 2, 3, 4, 1, 2, 3, 4])
    idx = rng.integers(0, 8, n)
    x = (feats[idx] + 0.3 * rng.standard_normal((n, 30, 20))).astype(np.float32)
    y = lab[idx]
    b = (0.5 * rng.standard_normal((bg, 30, 20)) - 20.0).astype(np.float32)
    return pcm, np.concatenate([x, b]), np.concatenate([y, np.zeros(bg, np.int64)])


def _recalibrate_bn(m, x):
    """set the BatchNormalization moving statistics to the training set's own, layer by layer (float64 oracle): twelve short epochs
    leave them far from converged, and the inference forward the int8 model is compared with uses them"""
    from oracle import model_oracle as mo
    om = mo.Model("simple_cnn_lite", m.num_classes)
    om.set_weights([np.asarray(w, np.float64) for w in m.get_weights()])
    h = x.astype(np.float64)[..., None]
    for l in om.layers[:-1]:
        if isinstance(l, mo.BatchNorm):
            flat = h.reshape(-1, l.c)
            l.moving_mean, l.moving_variance = flat.mean(0), flat.var(0)
        h = l.forward(h, False)
    m.set_weights([np.asarray(w, np.float32) for w in om.get_weights()])


def test_trained_lite_model_keeps_its_accuracy_at_int8(torch, golden):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    from kws_amd.quant import QuantizedCNNLite
    C = 5
    rng = np.random.default_rng(17)
    pcm, x, y = _task(golden, rng, 512, 128)
    m = KWSModel("simple_cnn_lite", C, seed=5)
    m.compile(optimizer=get_optimizer("adam", 2e-3, decay_type=None), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x[..., None], y, batch_size=128, epochs=12, verbose=0)
    assert h.history["accuracy"][-1] > 0.9, h.history["accuracy"]
    _recalibrate_bn(m, x)
    _, xt, yt = _task(golden, np.random.default_rng(23), 2000, 400)
    p32 = m.predict(xt)
    a32 = p32.argmax(-1)
    acc32 = (a32 == yt).mean()
    print("simple_cnn_lite fp32: held-out accuracy %.4f, training-set accuracy at inference %.4f"
          % (acc32, (m.predict(x).argmax(-1) == y).mean()))
    assert acc32 > 0.8, acc32                            # a float model worth quantizing: the comparisons below say something
    e32 = m.predict(pcm).argmax(-1)
    for method in ("max", "relu6"):
        qm = m.quantize(x, method=method, batch_size=300)
        assert isinstance(qm.quantized, QuantizedCNNLite)
        np.testing.assert_array_equal(qm.predict(pcm).argmax(-1), e32)          # the eight clips, raw audio in
        a8 = qm.predict_classes(xt)
        agree = (a8 == a32).mean()
        acc8 = (a8 == yt).mean()
        print("simple_cnn_lite int8 %s: agreement %.4f, accuracy %.4f (fp32 %.4f)" % (method, agree, acc8, acc32))
        assert agree >= 0.98, (method, agree)
        assert acc8 >= acc32 - 0.01, (method, acc8, acc32)
        loss8, eacc8 = qm.evaluate(xt[..., None], yt)
        assert abs(eacc8 - acc8) < 1e-9 and np.isfinite(loss8)


def _write_tree(root, golden, classes):
    rng = np.random.default_rng(2)
    src = {"background": None, "right": "pcm_right_1", "left": "pcm_left_1"}
    for cname in classes:
        d = os.path.join(root, "sounds", cname)
        os.makedirs(d)
        for i in range(4):
            if src[cname] is None:
                pcm = (300 * rng.standard_normal(16000)).astype(np.int16)
            else:
                pcm = np.clip(golden[src[cname]].astype(np.float64) * rng.uniform(0.6, 1.2) + 200 * rng.standard_normal(16000),
                              -32768, 32767).astype(np.int16)
            w = wave.open(os.path.join(d, "%d.wav" % i), "wb")
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(pcm.tobytes()); w.close()


def test_eval_py_int8_lite_end_to_end(torch, golden, tmp_path):
    from classifier.model import get_model
    from kws_amd import quant
    classes = ["background", "right", "left"]
    data = str(tmp_path / "data")
    _write_tree(data, golden, classes)
    cpath = str(tmp_path / "classes.txt")
    with open(cpath, "w") as f:
        f.write("\n".join(classes) + "\n")
    m = get_model("simple_cnn_lite", 3)
    wpath = str(tmp_path / "w.npz")
    m.save_weights(wpath)
    base = [sys.executable, os.path.join(PKG, "eval.py"), "--model_type", "simple_cnn_lite", "--weights_path", wpath, "--dataset_path",
            data, "--classes_path", cpath]
    from classifier.data import get_dataset
    get_dataset(data, classes)                          # the feature cache exists before either run, so both print the same lines
    plain = subprocess.run(base, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert plain.returncode == 0, plain.stderr
    qpath = str(tmp_path / "q.npz")
    out = subprocess.run(base + ["--int8", "--calib_samples", "5", "--save_quantized", qpath], capture_output=True, text=True, cwd=ROOT,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith(plain.stdout)          # the fp32 report is unchanged, the int8 one follows it
    tail = out.stdout[len(plain.stdout):]
    assert "int8 (max calibration, 5 clips):" in tail and "out of 12 samples" in tail and "argmax agreement" in tail
    assert "Saved int8 model" in tail
    q = quant.load(qpath)
    assert isinstance(q, quant.QuantizedCNNLite) and q.method == "max" and q.num_classes == 3


def test_quantized_stream_batch_takes_its_probabilities_from_the_int8_model(torch, qsetup):
    from classifier.params import pr
    from kws_amd.stream import StreamBatch
    from kws_amd.quant import QuantizedCNNLite, calibrate
    C = 5
    om = _weights(C, 11, shift=0.05, head_gain=4.0)
    dm = _device_model(om, C)
    q = QuantizedCNNLite.from_model(dm, calibrate(dm, _features(256, 12, scale=1.0)), "max")
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
