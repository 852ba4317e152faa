"""CPU tests of the KL (entropy) calibration (include/kws.h: kws_quant_kl_ranges, KWS_QUANT_KL, kws_model_calibrate_hist's checks):
the host KL search against the numpy restatement (tests/kl_ref.py), the quantizers under KWS_QUANT_KL against KWS_QUANT_MAX with the
same ranges, the .npz round trip of a kl snapshot and eval.py's option."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
C = 9
BINS = 2048


def _spec(kind="simple_cnn", classes=C):
    from kws_amd.model import ModelSpec
    return ModelSpec(kind, classes, 30, 20)


def _flat(spec, seed=0):
    rng = np.random.default_rng(seed)
    p = np.zeros(max(spec.param_count, 4), np.float32)
    s = np.zeros(max(spec.state_count, 4), np.float32)
    for t in spec.tensors:
        n, shp = t["name"], t["shape"]
        if n.endswith("/kernel"):
            w = rng.uniform(-1.0, 1.5, shp) / np.sqrt(int(np.prod(shp[:-1])))
        elif n.endswith("/gamma"):
            w = rng.uniform(0.5, 1.5, shp)
        elif n.endswith("/moving_variance"):
            w = rng.uniform(0.2, 3.0, shp)
        else:
            w = rng.normal(0.0, 0.3, shp)
        (p if t["trainable"] else s)[t["offset"]:t["offset"] + t["size"]] = np.asarray(w, np.float32).reshape(-1)
    return p, s


def _kl_ranges(hist, amax):
    from kws_amd import lib as _l
    h = np.ascontiguousarray(np.asarray(hist, np.uint64).reshape(-1, BINS))
    a = np.ascontiguousarray(np.asarray(amax, np.float32))
    r, b = np.full(a.size, -1.0, np.float32), np.full(a.size, -1, np.int32)
    rc = _l.get_lib().kws_quant_kl_ranges(h.ctypes.data, a.ctypes.data, a.size, r.ctypes.data, b.ctypes.data)
    return rc, r, b


def _binned(samples, amax):
    return kl_ref.histogram(np.asarray(samples, np.float32), amax)


def _seeded_histograms():
    rng = np.random.default_rng(0)
    out = []
    e = rng.exponential(1.0, 200000)
    out.append(("exponential", _binned(e, e.max()), e.max()))
    g = rng.normal(0.0, 1.0, 200000)
    out.append(("gaussian", _binned(g, np.abs(g).max()), np.abs(g).max()))
    tp = np.concatenate([rng.normal(1.0, 0.2, 100000), rng.normal(4.0, 0.3, 30000)])
    out.append(("two_peak", _binned(tp, np.abs(tp).max()), np.abs(tp).max()))
    lt = rng.standard_cauchy(100000)
    out.append(("long_tail", _binned(lt, np.abs(lt).max()), np.abs(lt).max()))
    sp = np.zeros(BINS, np.int64)                          # sparse: few occupied bins, many zeros between them
    idx = rng.choice(BINS, 40, replace=False)
    sp[idx] = rng.integers(1, 500, 40)
    out.append(("sparse", sp, 5.0))
    sp2 = np.zeros(BINS, np.int64)                         # a bulk with gaps, and isolated bins far above it
    sp2[:300:3] = rng.integers(50, 5000, 100)
    sp2[[900, 1500, 2047]] = [3, 1, 2]
    out.append(("sparse_tail", sp2, 2.5))
    relu = np.clip(rng.normal(0.5, 1.5, 300000), 0, 6)    # a post-ReLU6 tensor: a spike at 6
    out.append(("relu6", _binned(relu, relu.max()), relu.max()))
    return out


def _check_against_ref(h, amax, i_got, a_got):
    i_want, a_want = kl_ref.kl_search(h, amax)
    if i_got != i_want:                                    # only a tie may differ
        kl = kl_ref.kl_divergences(h)
        k1, k2 = kl[i_got - 128], kl[i_want - 128]
        assert np.isfinite(k1) and abs(k1 - k2) <= 1e-12 * max(abs(k1), abs(k2)), (i_got, i_want, k1, k2)
        a_want = np.float32(i_got * float(np.float32(amax)) / BINS)
    assert a_got.view(np.uint32) == np.float32(a_want).view(np.uint32), (a_got, a_want)


def test_kl_search_matches_the_restatement_on_seeded_histograms():
    cases = _seeded_histograms()
    hist = np.stack([c[1] for c in cases])
    amax = np.array([c[2] for c in cases], np.float32)
    rc, r, b = _kl_ranges(hist, amax)
    assert rc == 0
    for (name, h, a), i, A in zip(cases, b, r):
        _check_against_ref(h, a, int(i), np.float32(A))
        assert 128 <= i <= 2048, name
    # the shapes differ in how much they clip: the long tail is cut far below its maximum, the bulk-only histograms are not
    named = dict(zip([c[0] for c in cases], b))
    assert named["long_tail"] < 512 and named["sparse_tail"] < 900


def test_kl_search_hand_cases():
    amax = np.float32(8.0)
    one_low = np.zeros(BINS, np.int64)
    one_low[5] = 1000                                      # every i >= 128 gives KL = 0: the smallest, 128
    top = np.zeros(BINS, np.int64)
    top[2047] = 77                                         # any i < 2048 folds mass into an empty bin: i* = 2048, A = amax
    spike = np.zeros(BINS, np.int64)
    rng = np.random.default_rng(1)
    spike[:400] = rng.integers(1000, 2000, 400)
    spike[1990:2000] = 1                                   # ten outliers far above the bulk
    empty = np.zeros(BINS, np.int64)
    hist = np.stack([one_low, top, spike, empty])
    rc, r, b = _kl_ranges(hist, np.full(4, amax))
    assert rc == 0
    assert b[0] == 128 and r[0] == np.float32(128 * 8.0 / 2048)
    assert b[1] == 2048 and r[1] == amax
    assert b[2] < 1000 and r[2] < 0.5 * amax
    _check_against_ref(spike, amax, int(b[2]), np.float32(r[2]))
    assert b[3] == 0 and r[3] == 0.0
    # a zero maximum gives a zero range whatever the counts; bins_out may be NULL
    from kws_amd import lib as _l
    L = _l.get_lib()
    h = np.ascontiguousarray(spike.astype(np.uint64))
    a = np.zeros(1, np.float32)
    out = np.full(1, -1.0, np.float32)
    assert L.kws_quant_kl_ranges(h.ctypes.data, a.ctypes.data, 1, out.ctypes.data, None) == 0 and out[0] == 0.0


def test_kl_search_rejects_bad_arguments():
    from kws_amd import lib as _l
    L = _l.get_lib()
    h = np.zeros((2, BINS), np.uint64)
    out = np.zeros(2, np.float32)
    for bad in ([np.nan, 1.0], [1.0, -1.0], [np.inf, 1.0]):
        a = np.array(bad, np.float32)
        assert L.kws_quant_kl_ranges(h.ctypes.data, a.ctypes.data, 2, out.ctypes.data, None) == -1
    a = np.ones(2, np.float32)
    assert L.kws_quant_kl_ranges(None, a.ctypes.data, 2, out.ctypes.data, None) == -1
    assert L.kws_quant_kl_ranges(h.ctypes.data, a.ctypes.data, -1, out.ctypes.data, None) == -1
    assert L.kws_quant_kl_ranges(None, None, 0, None, None) == 0


@pytest.mark.parametrize("kind,cls_name,nt", [("simple_cnn", "QuantizedCNN", 6), ("simple_cnn_lite", "QuantizedCNNLite", 10)])
def test_kl_method_quantizes_like_max_with_the_same_ranges(kind, cls_name, nt):
    from kws_amd import lib as _l
    from kws_amd import quant
    cls = getattr(quant, cls_name)
    spec = _spec(kind)
    p, s = _flat(spec, seed=3)
    L = _l.get_lib()
    fn = getattr(L, cls._QUANTIZE)
    rng = np.random.default_rng(4)
    ranges = rng.uniform(0.3, 9.0, nt).astype(np.float32)
    ranges[3] = 0.0                                        # a 0 range: 6 (post-ReLU6) or 1 (u2 of the lite model)
    for r in (ranges, np.full(nt, 2.0, np.float32)):
        qm, qk = cls._STRUCT(), cls._STRUCT()
        assert fn(spec.handle, p.ctypes.data, s.ctypes.data, r.ctypes.data, _l.QUANT_MAX, ctypes.byref(qm)) == 0
        assert fn(spec.handle, p.ctypes.data, s.ctypes.data, r.ctypes.data, _l.QUANT_KL, ctypes.byref(qk)) == 0
        assert qm.method == 0 and qk.method == 2
        qk.method = 0
        assert ctypes.string_at(ctypes.addressof(qm), ctypes.sizeof(qm)) == ctypes.string_at(ctypes.addressof(qk), ctypes.sizeof(qk))
    qk = cls._STRUCT()
    assert fn(spec.handle, p.ctypes.data, s.ctypes.data, ranges.ctypes.data, _l.QUANT_KL, ctypes.byref(qk)) == 0
    A = np.ctypeslib.as_array(qk.amax)
    relu6 = [1, 2, 3, 4, 5] if nt == 6 else [2, 4, 6, 8, 9]
    for t in relu6:                                        # capped at 6, a 0 becoming 6
        assert A[t] == (6.0 if ranges[t] == 0 else min(float(ranges[t]), 6.0)), t
    if nt == 10:
        assert A[3] == 1.0 and all(A[t] == float(ranges[t]) for t in (1, 5, 7))
    assert A[0] == float(ranges[0])
    # the fallbacks and the invalid cases of max hold under kl
    bad_cases = [np.r_[0.0, np.ones(nt - 1)], np.r_[np.nan, np.ones(nt - 1)], np.r_[1.0, -0.5, np.ones(nt - 2)],
                 np.r_[np.ones(nt - 1), np.inf]]
    for bad in bad_cases:
        b = np.ascontiguousarray(bad, np.float32)
        assert fn(spec.handle, p.ctypes.data, s.ctypes.data, b.ctypes.data, _l.QUANT_KL, ctypes.byref(qk)) == -1, bad
    assert fn(spec.handle, p.ctypes.data, s.ctypes.data, ranges.ctypes.data, 3, ctypes.byref(qk)) == -1


@pytest.mark.parametrize("kind,cls_name,nt", [("simple_cnn", "QuantizedCNN", 6), ("simple_cnn_lite", "QuantizedCNNLite", 10)])
def test_from_histograms_and_the_kl_npz_round_trip(tmp_path, kind, cls_name, nt):
    from kws_amd import quant
    cls = getattr(quant, cls_name)
    spec = _spec(kind)
    p, s = _flat(spec, seed=6)
    rng = np.random.default_rng(7)
    vals = [np.abs(rng.standard_cauchy(20000)).astype(np.float32) * np.float32(rng.uniform(0.01, 0.1)) for _ in range(nt)]
    amax = np.array([v.max() for v in vals], np.float32)   # long tails: every range clips
    hist = np.stack([_binned(v, a) for v, a in zip(vals, amax)])
    q = cls.from_histograms(spec, p, s, amax, hist)
    assert q.method == "kl"
    ranges = quant.kl_ranges(hist, amax)
    assert ranges.dtype == np.float32 and ranges.shape == (nt,) and (ranges <= amax).all() and (ranges < 0.5 * amax).sum() >= nt // 2
    rc, r2, b2 = _kl_ranges(hist, amax)
    assert rc == 0 and np.array_equal(r2, ranges)
    for h, a, i, A in zip(hist, amax, b2, r2):
        _check_against_ref(h, a, int(i), np.float32(A))
    want = cls._quantize(spec, p, s, ranges, 0)            # the max rules on the KL ranges
    assert np.array_equal(q.arrays["amax"], want.arrays["amax"])
    path = str(tmp_path / "kl.npz")
    q.save(path)
    r = quant.load(path)
    assert type(r) is cls and r.method == "kl"
    assert ctypes.string_at(ctypes.addressof(q._q), ctypes.sizeof(q._q)) == ctypes.string_at(ctypes.addressof(r._q), ctypes.sizeof(r._q))
    with pytest.raises(ValueError) as e:
        cls.from_weights(spec, p, s, amax, "kl")
    assert "from_histograms" in str(e.value)


def test_eval_py_lists_kl():
    out = subprocess.run([sys.executable, os.path.join(PKG, "eval.py"), "-h"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "kl" in out.stdout.split("--quant_method")[1].split("--save_quantized")[0]


@pytest.mark.parametrize("kind", ["simple_gru", "simple_lstm"])
def test_histogram_pass_is_unsupported_for_other_models(kind):
    from kws_amd import lib as _l
    spec = _spec(kind)
    a = np.ones(10, np.float32)
    L = _l.get_lib()
    assert L.kws_model_calibrate_hist(spec.handle, None, 4, None, None, None, 0, a.ctypes.data, None, None) == -2
    assert L.kws_model_calibrate_hist(None, None, 4, None, None, None, 0, a.ctypes.data, None, None) == -1


def test_calibrate_kl_needs_a_re_iterable_input():
    from kws_amd import quant
    feats = iter([np.zeros((2, 30, 20), np.float32)])
    with pytest.raises(TypeError):
        quant.calibrate_kl(None, feats)
