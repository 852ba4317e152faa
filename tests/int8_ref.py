"""numpy restatement of the int8 simple_cnn contract of include/kws.h (kws_quantize_simple_cnn, kws_qmodel_forward).

quantize(): the host quantizer in float64, every per-channel constant rounded once to float32.
forward(): the integer network on the exported arrays, with the device's float32 epilogue (multiply and add rounded separately,
rint half to even), so its logits are bit-equal to the kernel's."""
import numpy as np

from oracle import model_oracle as mo

BN_EPS = float(np.float32(1e-3))     # the library's float kBnEps widened to double
CONV_SHAPES = ((3, 3, 1, 16), (3, 3, 16, 32), (3, 3, 32, 64), (3, 3, 64, 128))


def _weight_q(W):
    """per output channel (last axis) MAX_ABS: int8 codes and s_wc (float64)"""
    W = np.asarray(W, np.float32).astype(np.float64)
    W2 = W.reshape(-1, W.shape[-1])
    r = np.abs(W2).max(0)
    sw = np.where(r == 0, 1.0, r / 127.0)
    q = np.clip(np.rint(W2 / sw), -127, 127).astype(np.int8).reshape(W.shape)
    return q, sw


def ranges(amax, method="max"):
    a = np.asarray(amax, np.float32).astype(np.float64)
    A = a.copy()
    for t in range(1, 6):
        A[t] = 6.0 if method == "relu6" or a[t] == 0 else min(a[t], 6.0)
    return A


def quantize(weights, amax, method="max"):
    """weights: the 24 simple_cnn arrays in Keras get_weights() order; amax: the 6 calibrated maxima -> dict of the arrays
    QuantizedCNN.arrays exports"""
    w = [np.asarray(x, np.float32) for x in weights]
    A = ranges(amax, method)
    s = A / 127.0
    out = {"amax": A, "scale": s, "inv_s0": np.float32(1.0 / s[0])}
    for l in range(4):
        k, gamma, beta, mm, mv = w[5 * l:5 * l + 5]
        q, sw = _weight_q(k)
        g = gamma.astype(np.float64) / np.sqrt(mv.astype(np.float64) + BN_EPS)
        h = beta.astype(np.float64) - mm.astype(np.float64) * g
        out["conv_w%d" % (l + 1)] = q
        out["M%d" % (l + 1)] = (((s[l] * sw) * g) / s[l + 1]).astype(np.float32)
        out["B%d" % (l + 1)] = (h / s[l + 1]).astype(np.float32)
    dk, db, hk, hb = w[20:24]
    q, sw = _weight_q(dk)
    out["dense_w"] = q
    out["Md"] = ((s[4] * sw) / s[5]).astype(np.float32)
    out["Bd"] = (db.astype(np.float64) / s[5]).astype(np.float32)
    q, sw = _weight_q(hk)
    out["head_w"] = q
    out["Mh"] = (s[5] * sw).astype(np.float32)
    out["head_bias"] = hb.astype(np.float32)
    return out


def requant(acc, M, Bq):
    r = acc.astype(np.float32) * np.asarray(M, np.float32)
    r = r + np.asarray(Bq, np.float32)
    return np.clip(np.rint(r), 0, 127).astype(np.int64)


def _matmul(a, b):
    """exact integer product through float64 (every partial sum of int8 x int8 products stays far below 2^53)"""
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def _conv(codes, q, stride=1):
    cols, _ = mo.im2col(codes, 3, 3, stride)
    return _matmul(cols, q.reshape(-1, q.shape[-1]))


def _pool(x):
    H, W = x.shape[1] // 2, x.shape[2] // 2
    return np.maximum(np.maximum(x[:, 0:2 * H:2, 0:2 * W:2], x[:, 0:2 * H:2, 1:2 * W:2]),
                      np.maximum(x[:, 1:2 * H:2, 0:2 * W:2], x[:, 1:2 * H:2, 1:2 * W:2]))


def forward(arr, feat):
    """arr: QuantizedCNN.arrays (or quantize()'s dict); feat (B, 30, 20) float32 -> (logits float32, probs float32, argmax int32)"""
    return head(arr, trunk(arr, feat))


def trunk(arr, feat):
    """the network up to the Dense layer's codes (B, 128), int64"""
    x = np.asarray(feat, np.float32).reshape(-1, 30, 20, 1)
    c = np.clip(np.rint(x * np.float32(arr["inv_s0"])), -127, 127).astype(np.int64)
    c = _pool(requant(_conv(c, arr["conv_w1"]), arr["M1"], arr["B1"]))
    c = _pool(requant(_conv(c, arr["conv_w2"]), arr["M2"], arr["B2"]))
    c = requant(_conv(c, arr["conv_w3"], 2), arr["M3"], arr["B3"])
    c = _pool(requant(np.maximum(_conv(c, arr["conv_w4"]), 0), arr["M4"], arr["B4"]))
    c = c.reshape(c.shape[0], -1)
    return requant(_matmul(c, arr["dense_w"]), arr["Md"], arr["Bd"])


def head(arr, d):
    """the head on the Dense layer's codes d (B, 128) -> (logits, probs, argmax) as forward() returns them"""
    acc = _matmul(d, arr["head_w"])
    logits = acc.astype(np.float32) * np.asarray(arr["Mh"], np.float32) + np.asarray(arr["head_bias"], np.float32)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    probs = e * (np.float32(1.0) / e.sum(1, keepdims=True, dtype=np.float32))
    return logits.astype(np.float32), probs.astype(np.float32), logits.argmax(1).astype(np.int32)
