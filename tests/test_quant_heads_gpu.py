"""GPU tests of the int8 classifier heads (kws_quant.hip, kws_quant_lite.hip: three 16-column MFMA tiles, C <= 48) bit for bit against
the numpy integer restatements (tests/int8_ref.py, tests/int8_lite_ref.py): every class count around the tile edges, every tail of the
8-clip block, exactly tied classes, and edge models with negative, zero and saturating channels in every layer."""
import numpy as np
import pytest

import int8_lite_ref
import int8_ref
from head_cases import (BQ_CH, GAMMA0, NEG_GAMMA, ZERO_COL, centre_head, device_model, edge_weights, oracle_maxima, quant_features,
                        quant_weights, tie_columns, tie_pairs, with_classes)

pytestmark = pytest.mark.gpu

KINDS = ("simple_cnn", "simple_cnn_lite")
CLASSES = (2, 15, 16, 17, 31, 32, 33, 36, 47, 48)
REF = {"simple_cnn": int8_ref, "simple_cnn_lite": int8_lite_ref}
N = 4096


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _quantize(om, amax):
    from kws_amd.quant import QuantizedCNN, QuantizedCNNLite
    cls = QuantizedCNNLite if om.model_type == "simple_cnn_lite" else QuantizedCNN
    return cls.from_model(device_model(om), amax, "max")


@pytest.fixture(scope="module")
def base(torch):
    """per kind: a 48-class model with a centred head, its calibration, the features and the restatement's Dense codes (the trunk
    does not depend on C: every class count below is this trunk with the first C head columns)"""
    from kws_amd.quant import calibrate
    out = {}
    for kind in KINDS:
        lite = kind == "simple_cnn_lite"
        om = quant_weights(kind, 48, 7, shift=0.05, head_gain=4.0)
        feat = quant_features(N, 8, 3.0 if lite else 1.0)
        centre_head(om, feat[:512])
        amax = calibrate(device_model(om), feat[:1024])
        q = _quantize(om, amax)
        d = np.concatenate([REF[kind].trunk(q.arrays, feat[i:i + 512]) for i in range(0, N, 512)])
        out[kind] = om, amax, feat, d
    return out


def _check(q, x, ref, torch):
    """device logits bit-equal to the restatement's, probabilities within 1e-6, the arg-max equal on every clip (ties included)"""
    wl, wp, wa = ref
    lg, pr, am = (t.cpu().numpy() for t in q.forward(torch.from_numpy(x).cuda(), logits=True))
    assert lg.shape == wl.shape and am.dtype == np.int32
    bad = np.nonzero((lg.view(np.uint32) != wl.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "logits differ on %d clips, first %s: %s vs %s" % (bad.size, bad[:3], lg[bad[0]], wl[bad[0]])
    np.testing.assert_allclose(pr, wp, atol=1e-6, rtol=0)
    np.testing.assert_array_equal(am, wa)
    return lg, pr, am


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", CLASSES)
def test_int8_head_classes(torch, base, kind, C):
    om48, amax, feat, d = base[kind]
    q = _quantize(with_classes(om48, C), amax)
    ref = REF[kind].head(q.arrays, d)
    _check(q, feat[3:], tuple(r[3:] for r in ref), torch)   # 4093 clips from an odd one: no alignment to the clip group
    assert np.unique(ref[2]).size >= min(C, 8)              # many classes win somewhere
    if C == 48:
        for b in range(1, 9):                               # every tail residue of the 8-clip block
            _check(q, feat[b:2 * b], tuple(r[b:2 * b] for r in ref), torch)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [36, 48])
def test_int8_tied_classes(torch, base, kind, C):
    """copied head columns across the tile and lane edges: bitwise-equal logits and probabilities, the lower class as the arg-max"""
    om48, amax, feat, d = base[kind]
    om = with_classes(om48, C)
    pairs = tie_pairs(C)
    lg0 = REF[kind].head(_quantize(om, amax).arrays, d[:512])[0]
    tie_columns(om, pairs, boost=3.0 * float(lg0.std(0).mean()))
    q = _quantize(om, amax)
    ref = REF[kind].head(q.arrays, d)
    lg, pr, am = _check(q, feat, ref, torch)
    wins = np.zeros(N, bool)
    for i, j in pairs:
        assert np.array_equal(q.arrays["head_w"][:, i], q.arrays["head_w"][:, j])
        assert np.array_equal(lg[:, i].view(np.uint32), lg[:, j].view(np.uint32))
        assert np.array_equal(pr[:, i].view(np.uint32), pr[:, j].view(np.uint32))
        w = lg[:, i] == lg.max(-1)
        assert w.sum() >= 10, (i, j, w.sum())
        np.testing.assert_array_equal(am[w], i)
        wins |= w
    assert wins.mean() > 0.5


@pytest.fixture(scope="module")
def edge(torch):
    out = {}
    for kind in KINDS:
        lite = kind == "simple_cnn_lite"
        om = edge_weights(kind, 48, 21)
        feat = quant_features(1024, 22, 3.0 if lite else 1.0)
        centre_head(om, feat[:512])
        out[kind] = om, feat
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_int8_edge_model(torch, edge, kind):
    """negative gamma on several channels of every BatchNorm (M < 0 before each 2 x 2 max), gamma = 0 (M = 0) with mid-range,
    always-127 and always-0 codes, an all-zero weight column in every quantized layer (s_w = 1), lite pointwise biases at +-2^23:
    the calibration pass against the float64 oracle, the forward bit for bit against the restatement"""
    from kws_amd.quant import calibrate
    lite = kind == "simple_cnn_lite"
    om, feat = edge[kind]
    amax = calibrate(device_model(om), feat)
    np.testing.assert_allclose(amax, oracle_maxima(om, feat), rtol=1e-5, atol=0)
    q = _quantize(om, amax)
    a = q.arrays
    for l in range(1, 5):
        M, Bq = np.asarray(a["M%d" % l]), np.asarray(a["B%d" % l])
        assert (M[list(NEG_GAMMA)] < 0).all() and (M[list(GAMMA0)] == 0).all(), l
        assert Bq[GAMMA0[1]] >= 127.5 and Bq[GAMMA0[2]] <= -0.5, l          # codes 127 / 0 everywhere in those channels
        if lite:
            assert list(np.asarray(a["bq%d" % l])[list(BQ_CH)]) == [2 ** 23, -2 ** 23], l
            assert (np.asarray(a["pw_w%d" % l])[..., ZERO_COL] == 0).all()
            assert l == 1 or (np.asarray(a["dw_w%d" % l])[:, :, ZERO_COL] == 0).all()            # stage 1 has one input channel
        else:
            assert (np.asarray(a["conv_w%d" % l])[..., ZERO_COL] == 0).all()
    s = np.asarray(a["scale"])
    assert (np.asarray(a["dense_w"])[:, ZERO_COL] == 0).all() and (np.asarray(a["head_w"])[:, ZERO_COL] == 0).all()
    assert a["Md"][ZERO_COL] == np.float32(s[-2] / s[-1]) and a["Mh"][ZERO_COL] == np.float32(s[-1])      # s_w = 1
    ref = REF[kind].forward(a, feat)
    _check(q, feat, ref, torch)
    _check(q, feat[1:42], tuple(r[1:42] for r in ref), torch)


@pytest.mark.parametrize("kind", KINDS)
def test_int8_softmax_underflow(torch, edge, kind):
    """a head gain at which most probabilities are exactly 0 in float32"""
    om, feat = edge[kind]
    from kws_amd.quant import calibrate
    loud = with_classes(om, 48)
    ws = loud.get_weights()
    ws[-2], ws[-1] = ws[-2] * 3000.0, ws[-1] * 3000.0
    loud.set_weights(ws)
    q = _quantize(loud, calibrate(device_model(loud), feat))
    ref = REF[kind].forward(q.arrays, feat)
    _, pr, _ = _check(q, feat, ref, torch)
    assert (pr == 0).mean() > 0.5 and (ref[1] == 0).mean() > 0.5
