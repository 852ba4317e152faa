"""GPU tests of the KL (entropy) calibration of the int8 models (include/kws.h: kws_model_calibrate_hist, kws_quant_kl_ranges,
KWS_QUANT_KL; kws_amd.quant.histograms / calibrate_kl / from_model_histograms): the histogram pass against numpy and the float64
oracle, exact folding of batches, the int8 forwards bit for bit against the integer restatements on inputs that saturate every KL
range, accuracy after quantizing a trained model with kl, and eval.py --quant_method kl.  Both model kinds."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import int8_lite_ref
import int8_ref
import kl_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
KINDS = ["simple_cnn", "simple_cnn_lite"]
NT = {"simple_cnn": 6, "simple_cnn_lite": 10}
REF = {"simple_cnn": int8_ref, "simple_cnn_lite": int8_lite_ref}
SEP = (0, 4, 8, 11)                                      # the SeparableConv2D layers of the lite oracle model
ACT = (3, 7, 10, 14, 18)                                 # pool 1, pool 2, stage / conv 3's ReLU6, pool 4, Dense's ReLU6


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _weights(kind, C, seed, shift=0.05, head_gain=4.0):
    """oracle glorot weights made asymmetric, with non-trivial BatchNorm statistics (and biases), one negative gamma and a head with
    zero column sums scaled by `head_gain` (the recipe of the existing int8 tests)"""
    from oracle import model_oracle as mo
    om = mo.Model(kind, C).init_weights(seed)
    rng = np.random.default_rng(seed + 100)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n.endswith("kernel"):
            ws[i] = ws[i] * 1.3 + shift * np.abs(ws[i]).mean()
        elif n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.2 * rng.standard_normal(ws[i].shape)
    ws[-2] = (ws[-2] - ws[-2].mean(0)) * head_gain
    om.set_weights([np.asarray(w, np.float32).astype(np.float64) for w in ws])
    return om


def _device_model(om, kind, C):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(kind, C, 30, 20))
    dm.set_weights([w.astype(np.float32) for w in om.get_weights()])
    return dm


def _features(n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, 30, 20)) + 0.5 * rng.standard_normal((n, 1, 20))).astype(np.float32)


def _oracle_tensors(om, kind, feat):
    """the values of the T quantized tensors of the float64 oracle forward, in the order of amax"""
    x = feat.astype(np.float64)[..., None]
    out = [x]
    for i, l in enumerate(om.layers[:-1]):
        x = l.forward(x, False)
        if kind == "simple_cnn_lite" and i in SEP:
            out.append(l.cache[2])                       # u_l: the depthwise output
        if i in ACT:
            out.append(x)
    return out


def _setup(torch, kind, C=7, seed=1):
    om = _weights(kind, C, seed)
    return om, _device_model(om, kind, C)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 17, 4096])
def test_input_histogram_is_numpy_binning_exactly(torch, kind, B):
    from kws_amd.quant import calibrate, histograms
    om, dm = _setup(torch, kind)
    feat = _features(B, 3 + B)
    feat[0, 0, :5] = 0.0                                 # zeros are not counted
    amax = calibrate(dm, feat)
    hist = histograms(dm, torch.from_numpy(feat).cuda(), amax)
    assert hist.dtype == torch.int64 and hist.is_cuda and tuple(hist.shape) == (NT[kind], 2048)
    h = hist.cpu().numpy()
    want = kl_ref.histogram(feat, amax[0])
    assert np.array_equal(h[0], want)
    assert h[0].sum() == np.count_nonzero(feat) and h[0, 2047] >= 1


@pytest.mark.parametrize("kind", KINDS)
def test_histograms_fold_batches_exactly(torch, kind):
    from kws_amd.quant import calibrate, calibrate_kl, histograms
    om, dm = _setup(torch, kind, seed=2)
    feat = _features(300, 5)
    amax = calibrate(dm, feat)
    whole = histograms(dm, feat, amax)
    h = histograms(dm, feat[:137], amax)
    halves = histograms(dm, torch.from_numpy(feat[137:]).cuda(), amax, hist=h)
    assert halves is h and torch.equal(halves, whole)
    assert torch.equal(histograms(dm, [feat[:50], feat[50:120], feat[120:]], amax), whole)
    assert int(histograms(dm, feat[:0], amax).sum().item()) == 0
    a2, h2 = calibrate_kl(dm, [feat[:100], feat[100:]])
    assert np.array_equal(a2, amax) and torch.equal(h2, whole)
    with pytest.raises(TypeError):
        calibrate_kl(dm, (f for f in [feat]))


@pytest.mark.parametrize("kind", KINDS)
def test_deeper_histograms_match_the_oracle(torch, kind):
    from kws_amd.quant import calibrate, histograms
    om, dm = _setup(torch, kind, C=9, seed=4)
    feat = _features(256, 6, scale=1.0)
    amax = calibrate(dm, feat)
    h = histograms(dm, feat, amax).cpu().numpy()
    vals = _oracle_tensors(om, kind, feat)
    assert len(vals) == NT[kind]
    for t, v in enumerate(vals):
        if amax[t] == 0:
            assert h[t].sum() == 0, t
            continue
        assert h[t, 2047] >= 1, t                        # the histogram forward reaches the max pass's maximum
        n_got, n_want = int(h[t].sum()), int(np.count_nonzero(v))
        assert abs(n_got - n_want) <= 0.001 * n_want + 2, (t, n_got, n_want)
        want = kl_ref.histogram(np.asarray(v, np.float32), amax[t])
        l1 = int(np.abs(h[t] - want).sum())
        assert l1 <= 0.01 * n_want, (t, l1, n_want)


@pytest.fixture(scope="module", params=KINDS)
def saturated(request, torch):
    """a model quantized with kl on a calibration set holding two clips far out of range (16x), and inputs beyond every range"""
    from kws_amd import quant
    kind = request.param
    C = 11
    om = _weights(kind, C, 7)
    dm = _device_model(om, kind, C)
    cal = _features(1024, 8, scale=1.0)
    cal[[100, 700]] *= 16.0                              # two clips far out of range (eight at 4x leave A_0 at 0.8 amax_0)
    amax, hist = quant.calibrate_kl(dm, cal)
    q = quant.quantized_class(kind).from_model_histograms(dm, amax, hist)
    feat = _features(4096, 9, scale=12.0)                # 12x the bulk of the calibration set: beyond every range
    outs = [REF[kind].forward(q.arrays, feat[i:i + 1024]) for i in range(0, len(feat), 1024)]
    ref = tuple(np.concatenate([o[k] for o in outs]) for k in range(3))
    return kind, dm, q, amax, feat, ref


def test_kl_clips_the_outliers(torch, saturated):
    kind, dm, q, amax, feat, ref = saturated
    A = q.arrays["amax"]
    assert q.method == "kl"
    assert A[0] < 0.5 * amax[0], (A[0], amax[0])
    assert (np.abs(feat) > A[0]).mean() > 0.01           # the inputs saturate t0
    # and the deeper tensors: the evaluated clips exceed the calibrated ranges
    from kws_amd.quant import calibrate
    big = calibrate(dm, feat)
    assert (big[1:] > A[1:] * 0.999).all(), (big, A)


@pytest.mark.parametrize("B", [1, 17, 4096])
def test_saturating_int8_forward_is_bit_equal_to_the_restatement(torch, saturated, B):
    kind, dm, q, amax, feat, ref = saturated
    x = feat[-B:]
    lg, pr, am = q.forward(torch.from_numpy(x).cuda(), logits=True)
    torch.cuda.synchronize()
    lg, pr, am = lg.cpu().numpy(), pr.cpu().numpy(), am.cpu().numpy()
    wl, wp, wa = (r[-B:] for r in ref)
    bad = np.nonzero((lg.view(np.uint32) != wl.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "logits differ on %d clips, first %s: %s vs %s" % (bad.size, bad[:3], lg[bad[0]], wl[bad[0]])
    np.testing.assert_allclose(pr, wp, atol=1e-6, rtol=0)
    top2 = np.sort(wl, 1)[:, -2:]
    distinct = top2[:, 1] > top2[:, 0]
    np.testing.assert_array_equal(am[distinct], wa[distinct])
    if B > 1000:
        assert all(np.unique(wl[:, c]).size > 1000 for c in range(q.num_classes))


def _task(golden, rng, n, bg):
    """the separable task of the existing int8 tests: noisy copies of the eight example clips' features (labels 1..4) plus quiet
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
    """BatchNormalization moving statistics set to the training set's own (float64 oracle), as test_quant_lite_gpu.py does"""
    from oracle import model_oracle as mo
    om = mo.Model(m.model_type, m.num_classes)
    om.set_weights([np.asarray(w, np.float64) for w in m.get_weights()])
    h = x.astype(np.float64)[..., None]
    for l in om.layers[:-1]:
        if isinstance(l, mo.BatchNorm):
            flat = h.reshape(-1, l.c)
            l.moving_mean, l.moving_variance = flat.mean(0), flat.var(0)
        h = l.forward(h, False)
    m.set_weights([np.asarray(w, np.float32) for w in om.get_weights()])


@pytest.mark.parametrize("kind", KINDS)
def test_trained_model_keeps_its_accuracy_with_kl(torch, golden, kind):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    from kws_amd import quant
    C = 5
    rng = np.random.default_rng(17)
    pcm, x, y = _task(golden, rng, 512, 128)
    m = KWSModel(kind, C, seed=5)
    m.compile(optimizer=get_optimizer("adam", 2e-3, decay_type=None), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x[..., None], y, batch_size=128, epochs=12, verbose=0)
    assert h.history["accuracy"][-1] > 0.9, h.history["accuracy"]
    if kind == "simple_cnn_lite":
        _recalibrate_bn(m, x)
    _, xt, yt = _task(golden, np.random.default_rng(23), 2000, 400)
    a32 = m.predict(xt).argmax(-1)
    acc32 = (a32 == yt).mean()
    if kind == "simple_cnn_lite":
        assert acc32 > 0.8, acc32
    e32 = m.predict(pcm).argmax(-1)
    res = {}
    for method in ("max", "relu6", "kl"):
        qm = m.quantize(x, method=method, batch_size=300)
        a8 = qm.predict_classes(xt)
        res[method] = ((a8 == a32).mean(), (a8 == yt).mean(), np.array_equal(qm.predict(pcm).argmax(-1), e32), qm)
        print("%s int8 %s: agreement %.4f, accuracy %.4f (fp32 %.4f), ranges %s"
              % (kind, method, res[method][0], res[method][1], acc32, np.round(qm.quantized.arrays["amax"], 3).tolist()))
    agree, acc8, eight, qm = res["kl"]
    assert isinstance(qm.quantized, quant.quantized_class(kind)) and qm.quantized.method == "kl"
    assert eight                                         # the eight clips, raw audio in, keep their arg-max
    assert agree >= 0.98, agree
    assert acc8 >= acc32 - 0.01, (acc8, acc32)


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


@pytest.mark.parametrize("kind", KINDS)
def test_eval_py_int8_kl_end_to_end(torch, golden, tmp_path, kind):
    from classifier.data import get_dataset
    from classifier.model import get_model
    from kws_amd import quant
    classes = ["background", "right", "left"]
    data = str(tmp_path / "data")
    _write_tree(data, golden, classes)
    cpath = str(tmp_path / "classes.txt")
    with open(cpath, "w") as f:
        f.write("\n".join(classes) + "\n")
    m = get_model(kind, 3)
    wpath = str(tmp_path / "w.npz")
    m.save_weights(wpath)
    get_dataset(data, classes)
    qpath = str(tmp_path / "q.npz")
    cmd = [sys.executable, os.path.join(PKG, "eval.py"), "--model_type", kind, "--weights_path", wpath, "--dataset_path", data,
           "--classes_path", cpath, "--int8", "--quant_method", "kl", "--calib_samples", "5", "--save_quantized", qpath]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "int8 (kl calibration, 5 clips):" in out.stdout and "out of 12 samples" in out.stdout and "Saved int8 model" in out.stdout
    q = quant.load(qpath)
    assert isinstance(q, quant.quantized_class(kind)) and q.method == "kl" and q.num_classes == 3
