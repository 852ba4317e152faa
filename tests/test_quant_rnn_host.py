"""CPU tests of the dynamic-range int8 simple_gru / simple_lstm (include/kws.h: kws_quantize_simple_rnn, kws_qmodel_create_rnn;
kws_amd.quant.QuantizedRNN): codes and scales against the numpy restatement (tests/int8_rnn_ref.py) bit for bit, the scope and
argument checks of the new entry points, the .npz round trip and eval.py's flags."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import int8_rnn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("simple_gru", "simple_lstm")


def _spec(kind, classes=12, T=30, F=20):
    from kws_amd.model import ModelSpec
    return ModelSpec(kind, classes, T, F)


def _prefix(kind):
    return "gru_unit_0" if kind == "simple_gru" else "lstm_unit_0"


def _weights(spec, seed=0):
    """asymmetric random weights with an all-zero column in each quantized matrix"""
    rng = np.random.default_rng(seed)
    ws = []
    for t in spec.tensors:
        shp = t["shape"]
        if t["name"].endswith("kernel"):
            w = rng.uniform(-1.0, 1.5, shp) / np.sqrt(shp[0])
        else:
            w = rng.normal(0.0, 0.3, shp)
        ws.append(w.astype(np.float32))
    names = [t["name"] for t in spec.tensors]
    p = _prefix(spec.model_type)
    ws[names.index(p + "/kernel")][:, 5] = 0.0
    ws[names.index(p + "/recurrent_kernel")][:, 50] = 0.0
    ws[names.index("score_predict/kernel")][:, 1] = 0.0
    return ws


def _flat(spec, ws):
    p = np.zeros(max(spec.param_count, 4), np.float32)
    for t, w in zip(spec.tensors, ws):
        assert t["trainable"]
        p[t["offset"]:t["offset"] + t["size"]] = w.reshape(-1)
    return p


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("classes,T,F", [(12, 30, 20), (48, 128, 64), (2, 1, 7)])
def test_quantizer_matches_the_restatement_bit_for_bit(kind, classes, T, F):
    from kws_amd.quant import QuantizedRNN
    spec = _spec(kind, classes, T, F)
    ws = _weights(spec)
    q = QuantizedRNN.from_weights(spec, _flat(spec, ws))
    got, want = q.arrays, int8_rnn_ref.quantize(kind, ws)
    assert set(got) == set(want)
    for k, v in want.items():
        g = np.asarray(got[k])
        assert g.dtype == v.dtype and g.shape == v.shape, k
        assert np.array_equal(_bits(g), _bits(v)), k
    assert q.method == "dynamic" and q._q.method == 3 and q._q.n_steps == T and q._q.feature_size == F
    assert not got["kernel"][:, 5].any() and got["kernel_scale"][5] == 0          # an all-zero column: codes 0, scale 0
    assert not got["head_w"][:, 1].any() and got["head_scale"][1] == 0
    for k in ("kernel", "recurrent_kernel", "head_w"):
        nz = np.abs(got[k]).max(0)
        assert ((nz == 127) | (nz == 0)).all(), k                                   # the largest weight of a column maps to +-127


def test_dequantized_weights_lie_within_half_a_step():
    from kws_amd.quant import QuantizedRNN
    for kind in KINDS:
        spec = _spec(kind)
        ws = _weights(spec, seed=3)
        arr = QuantizedRNN.from_weights(spec, _flat(spec, ws)).arrays
        for w, k, ks in ((ws[0], "kernel", "kernel_scale"), (ws[1], "recurrent_kernel", "recurrent_scale"), (ws[3], "head_w", "head_scale")):
            s = arr[ks].astype(np.float64)
            err = np.abs(arr[k].astype(np.float64) * s - w.astype(np.float64))
            assert (err <= s / 2 * (1 + 1e-6) + 1e-12).all(), (kind, k)


def test_restatement_rows_follow_the_contract():
    """the row quantizer of the restatement: ties to even, the maximum at +-127, an all-zero row"""
    v = np.array([[1.0, -0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0], [127.0, 0.5, 1.5, -2.5]], np.float32)
    codes, s = int8_rnn_ref.rows(v)
    assert codes.tolist() == [[127, -64, 32, 0], [0, 0, 0, 0], [127, 0, 2, -2]]
    assert s[1] == 0 and s[0] == np.float32(1.0) / np.float32(127) and s[2] == np.float32(1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_more_than_64_features_are_unsupported(kind):
    """F = 65 is refused when the model is made (the recurrent kernels take F <= 64), before it can reach the quantizer"""
    from kws_amd import KwsError
    with pytest.raises(KwsError) as e:
        _spec(kind, 12, 30, 65)
    assert e.value.code == -2


@pytest.mark.parametrize("kind,classes,T,F", [("simple_cnn", 12, 30, 20), ("simple_cnn_lite", 12, 30, 20), ("simple_gru", 49, 30, 20),
                                              ("simple_lstm", 49, 30, 20), ("simple_gru", 12, 129, 20), ("simple_lstm", 12, 129, 20)])
def test_other_models_are_unsupported(kind, classes, T, F):
    from kws_amd import lib as _l
    spec = _spec(kind, classes, T, F)
    p = np.zeros(max(spec.param_count, 4), np.float32)
    L = _l.get_lib()
    q = _l.KwsQSimpleRnn()
    assert L.kws_quantize_simple_rnn(spec.handle, p.ctypes.data, ctypes.byref(q)) == -2
    h_out = ctypes.c_void_p()
    assert L.kws_qmodel_create_rnn(spec.handle, ctypes.byref(q), ctypes.byref(h_out)) == -2 and not h_out.value


@pytest.mark.parametrize("kind", KINDS)
def test_the_cnn_entry_points_still_refuse_the_recurrent_models(kind):
    from kws_amd import lib as _l
    spec = _spec(kind)
    p = np.zeros(max(spec.param_count, 4), np.float32)
    s = np.zeros(4, np.float32)
    a = np.ones(10, np.float32)
    L = _l.get_lib()
    q, ql = _l.KwsQSimpleCnn(), _l.KwsQSimpleCnnLite()
    assert L.kws_quantize_simple_cnn(spec.handle, p.ctypes.data, s.ctypes.data, a.ctypes.data, 0, ctypes.byref(q)) == -2
    assert L.kws_quantize_simple_cnn_lite(spec.handle, p.ctypes.data, s.ctypes.data, a.ctypes.data, 0, ctypes.byref(ql)) == -2
    h_out = ctypes.c_void_p()
    assert L.kws_qmodel_create(spec.handle, ctypes.byref(q), ctypes.byref(h_out)) == -2
    assert L.kws_qmodel_create_lite(spec.handle, ctypes.byref(ql), ctypes.byref(h_out)) == -2


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_weights_and_mismatched_snapshots_are_invalid(kind):
    from kws_amd import KwsError, lib as _l
    from kws_amd.quant import QuantizedRNN
    spec = _spec(kind)
    ws = _weights(spec)
    for i, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf)):
        w2 = [w.copy() for w in ws]
        w2[i].reshape(-1)[7 % w2[i].size] = bad
        with pytest.raises(KwsError) as e:
            QuantizedRNN.from_weights(spec, _flat(spec, w2))
        assert e.value.code == -1, i
    L = _l.get_lib()
    q = QuantizedRNN.from_weights(spec, _flat(spec, ws))
    h_out = ctypes.c_void_p()
    other = _spec(kind, classes=13)
    assert L.kws_qmodel_create_rnn(other.handle, ctypes.byref(q._q), ctypes.byref(h_out)) == -1 and not h_out.value
    q._q.method = 0
    assert L.kws_qmodel_create_rnn(spec.handle, ctypes.byref(q._q), ctypes.byref(h_out)) == -1 and not h_out.value
    with pytest.raises(ValueError):
        QuantizedRNN.from_weights(spec, _flat(spec, ws), "max")


def test_methods_are_tied_to_the_model_kind():
    from kws_amd.quant import QuantizedCNN, QuantizedCNNLite, QuantizedRNN, quantized_class
    assert quantized_class("simple_gru") is QuantizedRNN and quantized_class("simple_lstm") is QuantizedRNN
    for cls, kind, n in ((QuantizedCNN, "simple_cnn", 6), (QuantizedCNNLite, "simple_cnn_lite", 10)):
        spec = _spec(kind)
        with pytest.raises(ValueError):
            cls.from_weights(spec, np.zeros(spec.param_count, np.float32), np.zeros(spec.state_count, np.float32), np.ones(n, np.float32),
                             "dynamic")


@pytest.mark.parametrize("kind", KINDS)
def test_npz_round_trip_is_exact(kind, tmp_path):
    from kws_amd import quant
    spec = _spec(kind, classes=9, T=40, F=13)
    q = quant.QuantizedRNN.from_weights(spec, _flat(spec, _weights(spec, seed=5)))
    path = str(tmp_path / "int8.npz")
    q.save(path)
    for r in (quant.QuantizedRNN.load(path), quant.load(path)):
        assert isinstance(r, quant.QuantizedRNN)
        assert r.method == "dynamic" and r.num_classes == 9 and r.spec.model_type == kind
        assert (r.spec.n_features, r.spec.feature_size) == (40, 13)
        a, b = q.arrays, r.arrays
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert ctypes.string_at(ctypes.addressof(q._q), ctypes.sizeof(q._q)) == ctypes.string_at(ctypes.addressof(r._q),
                                                                                                  ctypes.sizeof(r._q))
    with np.load(path) as z:
        assert str(z["__meta__"][0]) == "kws_int8_%s/1" % kind
    with pytest.raises(ValueError):
        quant.QuantizedCNN.load(path)


def test_eval_py_lists_the_dynamic_method():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tf-keras-speech-commands_amd", "eval.py"), "-h"], capture_output=True,
                         text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    section = out.stdout.split("--quant_method")[1].split("--save_quantized")[0]
    assert "dynamic" in section and "kl" in section


def test_eval_py_refuses_a_calibrated_method_for_the_recurrent_models(tmp_path):
    """checked before any data is read: the paths need not exist"""
    base = [sys.executable, os.path.join(ROOT, "tf-keras-speech-commands_amd", "eval.py"), "--weights_path", "w.npz", "--dataset_path",
            str(tmp_path), "--classes_path", "c.txt", "--int8"]
    out = subprocess.run(base + ["--model_type", "simple_gru", "--quant_method", "max"], capture_output=True, text=True, cwd=ROOT,
                         timeout=300)
    assert out.returncode == 2 and "dynamic" in out.stderr
    out = subprocess.run(base + ["--model_type", "simple_cnn", "--quant_method", "dynamic"], capture_output=True, text=True, cwd=ROOT,
                         timeout=300)
    assert out.returncode == 2 and "dynamic" in out.stderr
