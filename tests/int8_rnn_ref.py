"""numpy restatement of the dynamic-range int8 simple_gru / simple_lstm contract of include/kws.h (kws_quantize_simple_rnn, and
kws_qmodel_forward on a kws_qmodel_create_rnn handle).

quantize(): the host quantizer in float64, the column scales rounded once to float32.
forward(): the dynamic rows, the integer products and the rescales in float32 exactly as the device computes them; the gate functions
in float64 (the device's sigmoidf_ / tanh_fast_ are hardware approximations, not reproducible here), with h and c rounded to float32
after every step as the device keeps them.  Where the gates saturate to exactly 0 or 1 the logits are bit-equal to the kernel's."""
import numpy as np

U = 48
GATES = {"simple_gru": 3, "simple_lstm": 4}
f32 = np.float32


def quantize_columns(W):
    """per output column (last axis) symmetric MAX_ABS in float64 -> (int8 codes, float32 scales; 0 for an all-zero column)"""
    W = np.asarray(W, np.float32).astype(np.float64)
    a = np.abs(W).max(0)
    s = a / 127.0
    q = np.where(a > 0, np.clip(np.rint(W / np.where(a > 0, s, 1.0)), -127, 127), 0).astype(np.int8)
    return q, s.astype(np.float32)


def quantize(kind, weights):
    """weights: [kernel (F, N), recurrent_kernel (48, N), bias, head kernel (48, C), head bias] (the model's Keras order) -> the dict
    QuantizedRNN.arrays exports"""
    k, rk, b, hk, hb = [np.asarray(w, np.float32) for w in weights]
    assert k.shape[1] == GATES[kind] * U
    out = {}
    out["kernel"], out["kernel_scale"] = quantize_columns(k)
    out["recurrent_kernel"], out["recurrent_scale"] = quantize_columns(rk)
    out["head_w"], out["head_scale"] = quantize_columns(hk)
    out["bias"] = b.copy()
    out["head_bias"] = hb.copy()
    return out


def rows(v):
    """dynamic quantization of each row of v (..., n) float32 -> (codes int64, scales float32 (...)).  m = max|v|; inv = 127.f / m
    (IEEE float32 division), code = clamp(rint(v * inv), -127, 127) (ties to even), s = m / 127.f; m == 0 gives codes 0, s = 0."""
    v = np.asarray(v, np.float32)
    m = np.abs(v).max(-1)
    live = m > 0
    inv = np.where(live, f32(127) / np.where(live, m, f32(1)), f32(0)).astype(np.float32)
    codes = np.clip(np.rint(v * inv[..., None]), -127, 127).astype(np.int64)
    return codes, (m / f32(127)).astype(np.float32)


def _matmul(a, b):
    """exact integer product through float64 (every partial sum stays far below 2^53)"""
    return (a.astype(np.float64) @ np.asarray(b).astype(np.float64)).astype(np.int64)


def _rescale(acc, s_row, s_col):
    """((float)acc * s_row) * s_col, each multiply rounded to float32"""
    return (acc.astype(np.float32) * s_row[:, None]) * np.asarray(s_col, np.float32)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def gate_noise(seed, amplitude=1e-6):
    """a gate_hook for final_state: every gate output moved by a draw uniform within +-amplitude, the absolute error include/kws.h
    allows the device's sigmoidf_ / tanh_fast_ (one generator per hook: the draws follow the order of the calls)"""
    rng = np.random.default_rng(seed)
    return lambda name, t, a, y: y + rng.uniform(-amplitude, amplitude, y.shape)


def final_state(kind, arr, feat, gate_hook=None, states=None):
    """the recurrence: feat (B, T, F) float32 -> h_T (B, 48) float32.
    gate_hook(name, t, a, y) -> y': called for every gate function of step t (GRU: "z", "r"; LSTM: "i", "f", "g", "o" and "tc", the tanh
    of the new cell state) with its float32 pre-activation a and its float64 output y (B, 48); what it returns is used in y's place.
    states: a list that receives h after every step.  With neither, the result is what it was without them, bit for bit."""
    hook = gate_hook if gate_hook is not None else lambda name, t, a, y: y
    sig = lambda name, t, a: hook(name, t, a, _sig(a))
    tanh = lambda name, t, a: hook(name, t, a, np.tanh(a.astype(np.float64)))
    x = np.asarray(feat, np.float32)
    B, T, _ = x.shape
    bias = np.asarray(arr["bias"], np.float32)
    h = np.zeros((B, U), np.float32)
    c = np.zeros((B, U), np.float32)
    with np.errstate(over="ignore"):
        for t in range(T):
            cx, sx = rows(x[:, t])
            ch, sh = rows(h)
            X = _rescale(_matmul(cx, arr["kernel"]), sx, arr["kernel_scale"])
            H = _rescale(_matmul(ch, arr["recurrent_kernel"]), sh, arr["recurrent_scale"])
            if kind == "simple_gru":
                mx, mh = X + bias[0], H + bias[1]
                z = sig("z", t, mx[:, :U] + mh[:, :U])
                r = sig("r", t, mx[:, U:2 * U] + mh[:, U:2 * U])
                hh = mx[:, 2 * U:].astype(np.float64) + r * mh[:, 2 * U:].astype(np.float64)
                h = (z * h + (1.0 - z) * hh).astype(np.float32)
            else:
                a = (X + H) + bias
                i, f = sig("i", t, a[:, :U]), sig("f", t, a[:, U:2 * U])
                g, o = tanh("g", t, a[:, 2 * U:3 * U]), sig("o", t, a[:, 3 * U:])
                c = (f * c + i * g).astype(np.float32)
                h = (o * tanh("tc", t, c)).astype(np.float32)
            if states is not None:
                states.append(h)
    return h


def head(arr, h):
    """the head on h_T (B, 48) float32 -> (logits, probs, argmax) as the kernel returns them"""
    ch, sh = rows(h)
    logits = _rescale(_matmul(ch, arr["head_w"]), sh, arr["head_scale"]) + np.asarray(arr["head_bias"], np.float32)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    probs = e * (np.float32(1.0) / e.sum(1, keepdims=True, dtype=np.float32))
    return logits.astype(np.float32), probs.astype(np.float32), logits.argmax(1).astype(np.int32)


def forward(kind, arr, feat, gate_hook=None):
    """arr: QuantizedRNN.arrays (or quantize()'s dict); feat (B, T, F) float32 -> (logits float32, probs float32, argmax int32)"""
    return head(arr, final_state(kind, arr, feat, gate_hook))


def float_forward(kind, weights, feat):
    """the unquantized model in float64 (Keras semantics, as the fp32 kernels compute it): feat (B, T, F) -> logits (B, C)"""
    k, rk, b, hk, hb = [np.asarray(w, np.float64) for w in weights]
    x = np.asarray(feat, np.float64)
    B, T, _ = x.shape
    h = np.zeros((B, U))
    c = np.zeros((B, U))
    with np.errstate(over="ignore"):
        for t in range(T):
            if kind == "simple_gru":
                mx, mh = x[:, t] @ k + b[0], h @ rk + b[1]
                z, r = _sig(mx[:, :U] + mh[:, :U]), _sig(mx[:, U:2 * U] + mh[:, U:2 * U])
                h = z * h + (1.0 - z) * (mx[:, 2 * U:] + r * mh[:, 2 * U:])
            else:
                a = x[:, t] @ k + h @ rk + b
                c = _sig(a[:, U:2 * U]) * c + _sig(a[:, :U]) * np.tanh(a[:, 2 * U:3 * U])
                h = _sig(a[:, 3 * U:]) * np.tanh(c)
    return h @ hk + hb
