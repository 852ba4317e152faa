"""int8 post-training quantization of simple_cnn and simple_cnn_lite (include/kws.h: kws_model_calibrate[_lite],
kws_quantize_simple_cnn[_lite], kws_qmodel_*).

The reference quantizes a trained model outside Python (the MNN quantizer with inference/MNN/configs/quantizeConfig.json, or
tools/model_converter/custom_tflite_convert.py --post_training_quantize) and measures it with eval.py.  Here:

    amax = calibrate(dm, feature_batches)                 # fp32 forward on the GPU, running maxima of the six quantized tensors
    q = QuantizedCNN.from_model(dm, amax, method="max")   # host quantizer (the contract of include/kws.h), uploaded to the device
    probs, argmax = q.forward(features)                   # ONE int8 kernel from features to probabilities
    q.save("model_int8.npz"); q = load("model_int8.npz")

Entropy (KL) calibration, the reference's deployment recipe ("feature_quantize_method": "KL"): a max pass, then a histogram pass over
the same clips, then the KL search on the host:

    amax, hist = calibrate_kl(dm, feature_batches)        # = calibrate(...), then histograms(dm, feature_batches, amax)
    q = QuantizedCNN.from_model_histograms(dm, amax, hist)    # ranges kl_ranges(hist, amax); q.method == "kl"

simple_cnn_lite: calibrate() returns its ten maxima (x and the depthwise outputs u1..u4 beside the activations) and QuantizedCNNLite
takes the place of QuantizedCNN, with the same interface.  A quantized model is a frozen snapshot of the weights it was made from.

simple_gru / simple_lstm: dynamic-range int8 (custom_tflite_convert.py --post_training_quantize), no calibration:

    q = QuantizedRNN.from_model(dm)                       # q.method == "dynamic"; forward / save / load as above"""
import ctypes

import numpy as np

from . import lib as _l

_SHAPES = {"conv_w1": (3, 3, 1, 16), "conv_w2": (3, 3, 16, 32), "conv_w3": (3, 3, 32, 64), "conv_w4": (3, 3, 64, 128),
           "dense_w": (256, 128)}
_EPILOGUE = ("M1", "B1", "M2", "B2", "M3", "B3", "M4", "B4", "Md", "Bd")
_FORMAT = "kws_int8_simple_cnn/1"
_LITE_CH = ((1, 16), (16, 32), (32, 64), (64, 128))
_LITE_SHAPES = dict([("dw_w%d" % (l + 1), (3, 3, ci, 1)) for l, (ci, co) in enumerate(_LITE_CH)] +
                    [("pw_w%d" % (l + 1), (1, 1, ci, co)) for l, (ci, co) in enumerate(_LITE_CH)] + [("dense_w", (256, 128))])
_LITE_EPILOGUE = ("bq1", "bq2", "bq3", "bq4", "Mu1", "Mu2", "Mu3", "Mu4") + _EPILOGUE
_LITE_FORMAT = "kws_int8_simple_cnn_lite/1"


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _l.KwsError(-3, "no HIP device visible to torch: int8 inference has no CPU fallback")
    return torch


def _as_feature_tensor(x, spec):
    torch = _torch()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    n = spec.n_features * spec.feature_size
    if t.numel() % n:
        raise ValueError("features must have shape (B, %d, %d[, 1])" % (spec.n_features, spec.feature_size))
    return t.reshape(t.numel() // n, spec.n_features, spec.feature_size).to(torch.float32).cuda().contiguous()


def calibrate(dm, feature_batches, amax=None):
    """Running maxima (numpy float32 (6,)) of t0..t5 -- max|x|, a1, a2, a3, a4, d -- of the fp32 inference forward of a simple_cnn
    DeviceModel over `feature_batches` (one (B, n_features, feature_size[, 1]) array / tensor, or an iterable of them).  `amax`: a
    CUDA float32 (6,) tensor to fold the batches into (the running maxima of earlier calls); a fresh zero one by default.
    A simple_cnn_lite DeviceModel gives ten maxima: max|x|, max|u1|, a1, max|u2|, a2, max|u3|, a3, max|u4|, a4, d (u_l = the depthwise
    output of stage l)."""
    torch = _torch()
    L = _l.get_lib()
    lite = dm.spec.model_type == "simple_cnn_lite"
    n = _l.QLITE_TENSORS if lite else _l.QUANT_TENSORS
    fn = L.kws_model_calibrate_lite if lite else L.kws_model_calibrate
    if amax is None:
        amax = torch.zeros((n,), dtype=torch.float32, device=dm.device)
    elif amax.dtype != torch.float32 or not amax.is_cuda or amax.numel() != n:
        raise ValueError("amax must be a CUDA float32 tensor of %d values" % n)
    if isinstance(feature_batches, (np.ndarray, torch.Tensor)):
        feature_batches = [feature_batches]
    for fb in feature_batches:
        f = _as_feature_tensor(fb, dm.spec)
        _l.check(fn(dm.spec.handle, f.data_ptr(), f.shape[0], dm.params.data_ptr(), dm.state.data_ptr(), None, 0,
                                       amax.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return amax.cpu().numpy()


def _n_tensors(dm):
    return _l.QLITE_TENSORS if dm.spec.model_type == "simple_cnn_lite" else _l.QUANT_TENSORS


def histograms(dm, feature_batches, amax, hist=None):
    """Running counts (CUDA int64 (T, 2048), T = 6 / 10) of the quantized tensors of the fp32 inference forward over `feature_batches`
    (as calibrate takes them), binned by the finished maxima `amax` of calibrate() over the same set (include/kws.h,
    kws_model_calibrate_hist: |v| * (2048 / amax_t) for every nonzero value).  `hist`: a tensor of earlier counts to add to (every
    call adds its batches exactly: halves fold to the whole); a fresh zero one by default."""
    torch = _torch()
    L = _l.get_lib()
    n = _n_tensors(dm)
    a = np.ascontiguousarray(np.asarray(amax, np.float32).reshape(-1))
    if a.size != n:
        raise ValueError("amax must hold %d values" % n)
    if hist is None:
        hist = torch.zeros((n, _l.QUANT_HIST_BINS), dtype=torch.int64, device=dm.device)
    elif hist.dtype != torch.int64 or not hist.is_cuda or tuple(hist.shape) != (n, _l.QUANT_HIST_BINS) or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous CUDA int64 tensor of shape (%d, %d)" % (n, _l.QUANT_HIST_BINS))
    if isinstance(feature_batches, (np.ndarray, torch.Tensor)):
        feature_batches = [feature_batches]
    for fb in feature_batches:
        f = _as_feature_tensor(fb, dm.spec)
        _l.check(L.kws_model_calibrate_hist(dm.spec.handle, f.data_ptr(), f.shape[0], dm.params.data_ptr(), dm.state.data_ptr(), None, 0,
                                            a.ctypes.data, hist.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return hist


def kl_ranges(hist, amax):
    """Host only: the KL ranges A_t (numpy float32 (T,)) of the counts `hist` ((T, 2048), a CUDA tensor or an array) binned by `amax`
    (kws_quant_kl_ranges: the smallest of the least-divergent clip points i*, A_t = i* amax_t / 2048)."""
    h = hist.cpu().numpy() if hasattr(hist, "cpu") else np.asarray(hist)
    h = np.ascontiguousarray(h.astype(np.uint64).reshape(-1, _l.QUANT_HIST_BINS))
    a = np.ascontiguousarray(np.asarray(amax, np.float32).reshape(-1))
    if a.size != h.shape[0]:
        raise ValueError("amax holds %d values for %d histograms" % (a.size, h.shape[0]))
    out = np.zeros(a.size, np.float32)
    _l.check(_l.get_lib().kws_quant_kl_ranges(h.ctypes.data, a.ctypes.data, a.size, out.ctypes.data, None))
    return out


def calibrate_kl(dm, feature_batches):
    """The two calibration passes of the KL method over `feature_batches` -> (amax, hist): calibrate(), then histograms() with its
    maxima.  The input is read twice, so it must be re-iterable: one array / tensor, or a list or tuple of them (TypeError for a
    one-shot iterator)."""
    import torch
    if not isinstance(feature_batches, (np.ndarray, torch.Tensor, list, tuple)):
        raise TypeError("calibrate_kl reads its input twice: pass an array, a tensor, or a list or tuple of them, not %s"
                        % type(feature_batches).__name__)
    amax = calibrate(dm, feature_batches)
    return amax, histograms(dm, feature_batches, amax)


class QuantizedCNN(object):
    """An int8 simple_cnn on the current HIP device (kws_qmodel).  Build it with from_model or load."""
    _STRUCT = _l.KwsQSimpleCnn
    _QUANTIZE, _CREATE = "kws_quantize_simple_cnn", "kws_qmodel_create"
    _NT = _l.QUANT_TENSORS
    _SHAPES, _EPILOGUE, _FORMAT = _SHAPES, _EPILOGUE, _FORMAT

    def __init__(self, spec, qstruct):
        self.spec = spec
        self._q = qstruct
        self._L = _l.get_lib()
        self._h = ctypes.c_void_p()
        self.device = None

    def _handle(self):
        """the device copy (kws_qmodel_create on the current device at the first forward: quantizing, arrays and save / load are
        host-only)"""
        if not self._h.value:
            torch = _torch()
            _l.check(getattr(self._L, self._CREATE)(self.spec.handle, ctypes.byref(self._q), ctypes.byref(self._h)))
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self._h

    @classmethod
    def from_weights(cls, spec, params, state, amax, method="max"):
        """Host only: quantize the flat float32 params / state buffers of a simple_cnn ModelSpec (the layout of spec.tensors) with the
        calibrated maxima `amax` (6 values); method "max" (the calibrated activation ranges, capped at 6) or "relu6" (every activation
        range 6)."""
        if method not in _l.QUANT_METHODS:
            raise ValueError("method must be one of %s%s" % (sorted(_l.QUANT_METHODS), "; the kl method needs histograms of the calibration"
                             " set: calibrate_kl, then from_histograms / from_model_histograms" if method == "kl" else ""))
        return cls._quantize(spec, params, state, amax, _l.QUANT_METHODS[method])

    @classmethod
    def from_histograms(cls, spec, params, state, amax, hist):
        """Host only: quantize as from_weights with the KL ranges of the calibration histograms `hist` (histograms() / calibrate_kl)
        binned by the maxima `amax`; the rules of "max" apply to those ranges and the snapshot records method "kl"."""
        return cls._quantize(spec, params, state, kl_ranges(hist, amax), _l.QUANT_KL)

    @classmethod
    def from_model_histograms(cls, dm, amax, hist):
        """Quantize the CURRENT weights of a DeviceModel with KL ranges (see from_histograms)"""
        return cls.from_histograms(dm.spec, dm.params.cpu().numpy(), dm.state.cpu().numpy(), amax, hist)

    @classmethod
    def _quantize(cls, spec, params, state, amax, code):
        p = np.ascontiguousarray(np.asarray(params, np.float32).reshape(-1))
        s = np.ascontiguousarray(np.asarray(state, np.float32).reshape(-1))
        a = np.ascontiguousarray(np.asarray(amax, np.float32).reshape(-1))
        if p.size < spec.param_count or s.size < spec.state_count:
            raise ValueError("params / state are shorter than the model's %d / %d floats" % (spec.param_count, spec.state_count))
        if a.size != cls._NT:
            raise ValueError("amax must hold %d values" % cls._NT)
        q = cls._STRUCT()
        _l.check(getattr(_l.get_lib(), cls._QUANTIZE)(spec.handle, p.ctypes.data, s.ctypes.data, a.ctypes.data, code, ctypes.byref(q)))
        return cls(spec, q)

    @classmethod
    def from_model(cls, dm, amax, method="max"):
        """Quantize the CURRENT weights of a simple_cnn DeviceModel (see from_weights)"""
        return cls.from_weights(dm.spec, dm.params.cpu().numpy(), dm.state.cpu().numpy(), amax, method)

    @property
    def num_classes(self):
        return self.spec.num_classes

    @property
    def method(self):
        return {v: k for k, v in _l.QUANT_SNAPSHOT_METHODS.items()}[self._q.method]

    @property
    def arrays(self):
        """numpy views of the quantized model: int8 weights in Keras shapes, the fp32 epilogue constants, inv_s0, the scales s_0..s_5
        and the ranges A_0..A_5 (views into the host copy; the device copy is made at the first forward)."""
        q, C = self._q, self.spec.num_classes
        out = {}
        for n, shp in self._SHAPES.items():
            out[n] = np.ctypeslib.as_array(getattr(q, n)).reshape(shp)
        out["head_w"] = np.ctypeslib.as_array(q.head_w)[:128 * C].reshape(128, C)
        for n in self._EPILOGUE:
            out[n] = np.ctypeslib.as_array(getattr(q, n))
        out["Mh"] = np.ctypeslib.as_array(q.Mh)[:C]
        out["head_bias"] = np.ctypeslib.as_array(q.head_bias)[:C]
        out["inv_s0"] = np.float32(q.inv_s0)
        out["scale"] = np.ctypeslib.as_array(q.scale)
        out["amax"] = np.ctypeslib.as_array(q.amax)
        return out

    def _launch(self, feat, B, logits, probs, argmax):
        torch = _torch()
        ptr = lambda t: t.data_ptr() if t is not None else None
        _l.check(self._L.kws_qmodel_forward(self._handle(), feat.data_ptr(), int(B), None, 0, ptr(logits), ptr(probs), ptr(argmax),
                                            torch.cuda.current_stream().cuda_stream))

    def forward(self, features, logits=False):
        """features (B, n_features, feature_size[, 1]) -> (probs, argmax) CUDA tensors, or (logits, probs, argmax) with logits=True"""
        torch = _torch()
        f = _as_feature_tensor(features, self.spec)
        B, C = f.shape[0], self.spec.num_classes
        lg = torch.empty((B, C), dtype=torch.float32, device=f.device) if logits else None
        probs = torch.empty((B, C), dtype=torch.float32, device=f.device)
        am = torch.empty((B,), dtype=torch.int32, device=f.device)
        self._launch(f, B, lg, probs, am)
        return (lg, probs, am) if logits else (probs, am)

    __call__ = forward

    def save(self, path):
        """.npz (the project's checkpoint format): the arrays above plus the model's geometry; load() rebuilds the model from them"""
        arrays = {k: np.asarray(v) for k, v in self.arrays.items()}
        arrays["__meta__"] = np.array([self._FORMAT, self.spec.model_type, str(self.spec.num_classes), str(self.spec.n_features),
                                       str(self.spec.feature_size), self.method])
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path):
        """a QuantizedCNN from a file save() wrote (bit-identical arrays; the device copy is made by kws_qmodel_create, as for a
        freshly quantized model)"""
        from .model import ModelSpec
        z = np.load(path, allow_pickle=False)
        meta = [str(v) for v in z["__meta__"]]
        if meta[0] != cls._FORMAT:
            raise ValueError("%s is not a quantized %s checkpoint" % (path, cls._FORMAT.split("/")[0][9:]))
        spec = ModelSpec(meta[1], int(meta[2]), int(meta[3]), int(meta[4]))
        C = spec.num_classes
        q = cls._STRUCT()
        q.num_classes = C
        q.method = _l.QUANT_SNAPSHOT_METHODS[meta[5]]
        q.inv_s0 = float(z["inv_s0"])
        for n in cls._SHAPES:
            np.ctypeslib.as_array(getattr(q, n))[:] = z[n].reshape(-1)
        np.ctypeslib.as_array(q.head_w)[:128 * C] = z["head_w"].reshape(-1)
        for n in cls._EPILOGUE:
            np.ctypeslib.as_array(getattr(q, n))[:] = z[n]
        np.ctypeslib.as_array(q.Mh)[:C] = z["Mh"]
        np.ctypeslib.as_array(q.head_bias)[:C] = z["head_bias"]
        np.ctypeslib.as_array(q.scale)[:] = z["scale"]
        np.ctypeslib.as_array(q.amax)[:] = z["amax"]
        return cls(spec, q)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.kws_qmodel_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuantizedCNNLite(QuantizedCNN):
    """An int8 simple_cnn_lite on the current HIP device (kws_qmodel_create_lite; kws_qmodel_forward runs its one-kernel forward).
    The interface of QuantizedCNN; from_weights takes the ten maxima calibrate() returns for a simple_cnn_lite model, arrays adds the
    depthwise / pointwise codes (dw_w*, pw_w*), the int32 pointwise biases bq* and the depthwise multipliers Mu*."""
    _STRUCT = _l.KwsQSimpleCnnLite
    _QUANTIZE, _CREATE = "kws_quantize_simple_cnn_lite", "kws_qmodel_create_lite"
    _NT = _l.QLITE_TENSORS
    _SHAPES, _EPILOGUE, _FORMAT = _LITE_SHAPES, _LITE_EPILOGUE, _LITE_FORMAT


_RNN_FORMATS = {"simple_gru": "kws_int8_simple_gru/1", "simple_lstm": "kws_int8_simple_lstm/1"}
_RNN_GATES = {"simple_gru": 3, "simple_lstm": 4}


class QuantizedRNN(QuantizedCNN):
    """A dynamic-range int8 simple_gru / simple_lstm on the current HIP device (kws_quantize_simple_rnn, kws_qmodel_create_rnn): int8
    weights, every matrix input quantized per row on the fly, fp32 gates -- what custom_tflite_convert.py --post_training_quantize gives
    the reference's recurrent models.  No calibration: from_weights / from_model take the float parameters alone, and method is always
    "dynamic".  forward, arrays, save, load and close as QuantizedCNN's; the .npz formats are kws_int8_simple_gru/1 and
    kws_int8_simple_lstm/1."""
    _STRUCT = _l.KwsQSimpleRnn
    _CREATE = "kws_qmodel_create_rnn"
    _FORMAT = None
    _FORMATS = tuple(_RNN_FORMATS.values())

    @classmethod
    def from_weights(cls, spec, params, method="dynamic"):
        """Host only: quantize the flat float32 params buffer of a simple_gru / simple_lstm ModelSpec (the layout of spec.tensors)"""
        if method != "dynamic":
            raise ValueError("simple_gru / simple_lstm quantize with method 'dynamic' (dynamic-range int8) only, not %r" % (method,))
        p = np.ascontiguousarray(np.asarray(params, np.float32).reshape(-1))
        if p.size < spec.param_count:
            raise ValueError("params are shorter than the model's %d floats" % spec.param_count)
        q = cls._STRUCT()
        _l.check(_l.get_lib().kws_quantize_simple_rnn(spec.handle, p.ctypes.data, ctypes.byref(q)))
        return cls(spec, q)

    @classmethod
    def from_model(cls, dm, method="dynamic"):
        """Quantize the CURRENT weights of a simple_gru / simple_lstm DeviceModel (see from_weights)"""
        return cls.from_weights(dm.spec, dm.params.cpu().numpy(), method)

    @classmethod
    def from_histograms(cls, *args, **kwargs):
        raise ValueError("dynamic-range int8 quantization takes no calibration")

    @classmethod
    def from_model_histograms(cls, *args, **kwargs):
        raise ValueError("dynamic-range int8 quantization takes no calibration")

    @property
    def method(self):
        return "dynamic"

    @property
    def arrays(self):
        """numpy views of the host copy: the int8 kernel (F, N), recurrent_kernel (48, N) and head_w (48, C), their fp32 column scales
        kernel_scale, recurrent_scale, head_scale, and the fp32 biases (the GRU's (2, N), the LSTM's (N,), head_bias (C,))"""
        q, C = self._q, self.spec.num_classes
        G, F = _RNN_GATES[self.spec.model_type], self.spec.feature_size
        N, U = G * _l.QRNN_UNITS, _l.QRNN_UNITS
        a = lambda n: np.ctypeslib.as_array(getattr(q, n))
        return {"kernel": a("kernel")[:F * N].reshape(F, N), "recurrent_kernel": a("recurrent_kernel")[:U * N].reshape(U, N),
                "head_w": a("head_w")[:U * C].reshape(U, C), "kernel_scale": a("kernel_scale")[:N],
                "recurrent_scale": a("recurrent_scale")[:N], "bias": a("bias")[:2 * N].reshape(2, N) if G == 3 else a("bias")[:N],
                "head_scale": a("head_scale")[:C], "head_bias": a("head_bias")[:C]}

    def save(self, path):
        """.npz: the arrays above plus the model's geometry; load() rebuilds the model from them"""
        arrays = {k: np.asarray(v) for k, v in self.arrays.items()}
        arrays["__meta__"] = np.array([_RNN_FORMATS[self.spec.model_type], self.spec.model_type, str(self.spec.num_classes),
                                       str(self.spec.n_features), str(self.spec.feature_size), self.method])
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path):
        """a QuantizedRNN from a file save() wrote (bit-identical arrays)"""
        from .model import ModelSpec
        z = np.load(path, allow_pickle=False)
        meta = [str(v) for v in z["__meta__"]]
        if meta[0] not in cls._FORMATS or _RNN_FORMATS.get(meta[1]) != meta[0] or meta[5] != "dynamic":
            raise ValueError("%s is not a quantized simple_gru / simple_lstm checkpoint" % path)
        spec = ModelSpec(meta[1], int(meta[2]), int(meta[3]), int(meta[4]))
        q = cls._STRUCT()
        q.kind, q.num_classes = _l.MODEL_KINDS[meta[1]], spec.num_classes
        q.n_steps, q.feature_size, q.method = spec.n_features, spec.feature_size, _l.QUANT_DYNAMIC
        out = cls(spec, q)
        for k, v in out.arrays.items():
            v[...] = z[k]
        return out


_CLASSES = {"simple_cnn": QuantizedCNN, "simple_cnn_lite": QuantizedCNNLite, "simple_gru": QuantizedRNN, "simple_lstm": QuantizedRNN}


def quantized_class(model_type):
    """the quantized class of a model type (ValueError for the types int8 does not cover)"""
    if model_type not in _CLASSES:
        raise ValueError("int8 quantization covers %s, not %s" % (", ".join(sorted(_CLASSES)), model_type))
    return _CLASSES[model_type]


def load(path):
    """a QuantizedCNN, QuantizedCNNLite or QuantizedRNN from a file save() wrote, chosen by the file's format"""
    with np.load(path, allow_pickle=False) as z:
        fmt = str(z["__meta__"][0])
    for cls in _CLASSES.values():
        if fmt == cls._FORMAT or fmt in getattr(cls, "_FORMATS", ()):
            return cls.load(path)
    raise ValueError("%s is not a quantized model checkpoint (format %r)" % (path, fmt))
