"""numpy restatement of the int8 simple_cnn_lite contract of include/kws.h (kws_quantize_simple_cnn_lite, kws_qmodel_forward).

quantize(): the host quantizer in float64, every per-channel constant rounded once to float32.
forward(): the integer network on the exported arrays, with the device's float32 epilogue (multiply and add rounded separately,
rint half to even), so its logits are bit-equal to the kernel's."""
import numpy as np

from oracle import model_oracle as mo

from int8_ref import BN_EPS, _weight_q, _matmul, _pool, head, requant

CIN, COUT = (1, 16, 32, 64), (16, 32, 64, 128)
BQ_MAX = 2.0 ** 23


def ranges(amax, method="max"):
    """A_0..A_9: x as calibrated, u_l (odd t) as calibrated with 0 -> 1, a1..a4 and d capped at 6 with 0 -> 6 (6 for "relu6")"""
    a = np.asarray(amax, np.float32).astype(np.float64)
    A = a.copy()
    for t in range(1, 10):
        if t % 2 == 1 and t != 9:
            A[t] = 1.0 if a[t] == 0 else a[t]
        else:
            A[t] = 6.0 if method == "relu6" or a[t] == 0 else min(a[t], 6.0)
    return A


def quantize(weights, amax, method="max"):
    """weights: the 32 simple_cnn_lite arrays in Keras get_weights() order (per stage depthwise, pointwise, bias, gamma, beta, moving
    mean, moving variance; then Dense and head); amax: the 10 calibrated maxima -> dict of the arrays QuantizedCNNLite.arrays exports"""
    w = [np.asarray(x, np.float32) for x in weights]
    A = ranges(amax, method)
    s = A / 127.0
    out = {"amax": A, "scale": s, "inv_s0": np.float32(1.0 / s[0])}
    for l in range(4):
        dwk, pwk, bias, gamma, beta, mm, mv = w[7 * l:7 * l + 7]
        s_in, s_u, s_out = s[2 * l], s[2 * l + 1], s[2 * l + 2]
        qd, swd = _weight_q(dwk.reshape(9, CIN[l]))
        qp, swp = _weight_q(pwk.reshape(CIN[l], COUT[l]))
        out["dw_w%d" % (l + 1)] = qd.reshape(dwk.shape)
        out["pw_w%d" % (l + 1)] = qp.reshape(pwk.shape)
        out["Mu%d" % (l + 1)] = ((s_in * swd) / s_u).astype(np.float32)
        out["bq%d" % (l + 1)] = np.clip(np.rint(bias.astype(np.float64) / (s_u * swp)), -BQ_MAX, BQ_MAX).astype(np.int32)
        g = gamma.astype(np.float64) / np.sqrt(mv.astype(np.float64) + BN_EPS)
        h = beta.astype(np.float64) - mm.astype(np.float64) * g
        out["M%d" % (l + 1)] = (((s_u * swp) * g) / s_out).astype(np.float32)
        out["B%d" % (l + 1)] = (h / s_out).astype(np.float32)
    dk, db, hk, hb = w[28:32]
    q, sw = _weight_q(dk)
    out["dense_w"] = q
    out["Md"] = ((s[8] * sw) / s[9]).astype(np.float32)
    out["Bd"] = (db.astype(np.float64) / s[9]).astype(np.float32)
    q, sw = _weight_q(hk)
    out["head_w"] = q
    out["Mh"] = (s[9] * sw).astype(np.float32)
    out["head_bias"] = hb.astype(np.float32)
    return out


def requant_u(acc, Mu):
    r = acc.astype(np.float32) * np.asarray(Mu, np.float32)
    return np.clip(np.rint(r), -127, 127).astype(np.int64)


def _depthwise(codes, qdw, stride=1):
    """exact integer depthwise 3 x 3 ('same'; stride 2 pads 1 before and 1 after at the default geometry)"""
    cols, _ = mo.im2col(codes, 3, 3, stride)
    B, Ho, Wo, _ = cols.shape
    C = codes.shape[-1]
    c5 = cols.reshape(B, Ho, Wo, 9, C).astype(np.int64)
    return (c5 * np.asarray(qdw, np.int64).reshape(1, 1, 1, 9, C)).sum(3)


def _stage(arr, l, c, stride=1, relu=False):
    u = requant_u(_depthwise(c, arr["dw_w%d" % l], stride), arr["Mu%d" % l])
    acc = _matmul(u, np.asarray(arr["pw_w%d" % l]).reshape(u.shape[-1], -1)) + np.asarray(arr["bq%d" % l], np.int64)
    if relu:
        acc = np.maximum(acc, 0)
    return requant(acc, arr["M%d" % l], arr["B%d" % l])


def forward(arr, feat):
    """arr: QuantizedCNNLite.arrays (or quantize()'s dict); feat (B, 30, 20) float32 -> (logits float32, probs float32, argmax int32)"""
    return head(arr, trunk(arr, feat))


def trunk(arr, feat):
    """the network up to the Dense layer's codes (B, 128), int64"""
    x = np.asarray(feat, np.float32).reshape(-1, 30, 20, 1)
    c = np.clip(np.rint(x * np.float32(arr["inv_s0"])), -127, 127).astype(np.int64)
    c = _pool(_stage(arr, 1, c))
    c = _pool(_stage(arr, 2, c))
    c = _stage(arr, 3, c, stride=2, relu=True)
    c = _pool(_stage(arr, 4, c, relu=True))
    c = c.reshape(c.shape[0], -1)
    return requant(_matmul(c, arr["dense_w"]), arr["Md"], arr["Bd"])
