"""Model builders shared by the classifier-head tests (tests/test_heads_gpu.py, tests/test_quant_heads_gpu.py): float models with a
centred head, the head-dispatch formulas of the library (kws_model.hip: run_head, run_head_bwd; kws_cnn_plan.h: CnnPlan::fused_tail), tied head columns,
and the int8 test models of tests/test_quant_gpu.py and tests/test_quant_lite_gpu.py with their edge-case variants."""
import numpy as np

from oracle import model_oracle as mo

SEP = (0, 4, 8, 11)                                   # the SeparableConv2D layers of the oracle simple_cnn_lite


# ---- head dispatch (the formulas of kws_model.hip) ------------------------------------------------------------------
def head_forms(kind, K, C, matrix_bf16=True):
    """which head kernels a model of `kind` with K head inputs and C classes runs (default 30 x 20 geometry)"""
    return dict(
        fast_fwd=64 * (K + 1) + 4 * C * (K + 16) <= 60 * 1024,       # run_head: head_fwd_fast_kernel, else head_fwd_kernel
        mfma_bwd=K % 16 == 0 and K <= 128 and C <= 48,               # run_head_bwd: head_bwd_mfma_kernel, else head_bwd_kernel
        fused_tail=kind == "simple_cnn" and matrix_bf16 and C <= 48,  # CnnPlan::fused_tail: inference in infer_tail_kernel
        slow_lds=64 * (K + C))                                      # dynamic LDS of head_fwd_kernel / head_bwd_kernel


def head_inputs(kind):
    return 48 if kind in ("simple_gru", "simple_lstm") else 128


# ---- float models -----------------------------------------------------------------------------------------------------
def features(B, seed, n_features=30, feature_size=20):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, n_features, feature_size)) * 3.0
    x[..., 0] -= 10.0   # MFCC-like: a large negative c0 column
    return x.astype(np.float32)


def penultimate(om, x):
    """the head's input (float64, inference mode)"""
    h = np.asarray(x, np.float64)
    if om.input_rank == 4:
        h = h[..., None]
    for l in om.layers[:-1]:
        h = l.forward(h, False)
    return h


def float_model(kind, C, seed=0, spread=1.5, n_features=30, feature_size=20):
    """oracle weights as tests/test_model_gpu.py's build() perturbs them, BatchNorm moving statistics near those of a feature batch
    (so that inference and training see activations of the same scale), and a head centred on the batch (bias = -mean logit) and
    scaled to logits of standard deviation `spread` over the clips, so that many classes win somewhere; rounded to the device's
    float32"""
    om = mo.Model(kind, C, n_features=n_features, feature_size=feature_size).init_weights(seed)
    rng = np.random.default_rng(seed + 1)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    om.set_weights(ws)
    h = features(256, seed + 2, n_features, feature_size).astype(np.float64)
    h = h[..., None] if om.input_rank == 4 else h
    for l in om.layers[:-1]:
        if isinstance(l, mo.BatchNorm):
            flat = h.reshape(-1, l.c)
            l.moving_mean, l.moving_variance = flat.mean(0), flat.var(0) * rng.uniform(0.8, 1.25, l.c)
        h = l.forward(h, False)
    ws = om.get_weights()
    ws[-2] = ws[-2] * (spread / ((h - h.mean(0)) @ ws[-2]).std(0).mean())
    ws[-1] = -(h.mean(0) @ ws[-2])
    om.set_weights([np.asarray(w, np.float32) for w in ws])
    return om


def centre_head(om, x):
    ws = om.get_weights()
    ws[-1] = -(penultimate(om, x).mean(0) @ ws[-2])
    om.set_weights([np.asarray(w, np.float32) for w in ws])


def device_model(om, kind=None, C=None):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(kind or om.model_type, C or om.num_classes, om.n_features, om.feature_size))
    dm.set_weights([w.astype(np.float32) for w in om.get_weights()])
    return dm


# ---- exact ties ---------------------------------------------------------------------------------------------------------
def tie_pairs(C):
    """column pairs (i < j) that straddle lane and tile boundaries of the 16-column head layouts: 15 | 16 and 31 | 32 (tile edges),
    2 / 18 and 21 / 37 (the same lane of two tiles) and 0 / C - 1"""
    pairs = [(15, 16), (2, 18), (0, C - 1)]
    if C > 32:
        pairs.append((31, 32))
    if C > 38:
        pairs.append((21, 37))
    return pairs


def tie_columns(om, pairs, boost):
    """column j := column i (kernel and bias) for every pair, and both biases raised by `boost`, so that the pairs win most clips"""
    ws = om.get_weights()
    hk, hb = ws[-2].copy(), ws[-1].copy()
    for i, j in pairs:
        hb[i] += boost
        hk[:, j], hb[j] = hk[:, i], hb[i]
    ws[-2], ws[-1] = hk, hb
    om.set_weights([np.asarray(w, np.float32) for w in ws])


def with_classes(om, C):
    """the same trunk with the first C head columns"""
    ws = om.get_weights()
    ws[-2], ws[-1] = ws[-2][:, :C], ws[-1][:C]
    out = mo.Model(om.model_type, C)
    out.set_weights(ws)
    return out


# ---- int8 test models (tests/test_quant_gpu.py, tests/test_quant_lite_gpu.py) -------------------------------------------
def quant_weights(kind, C, seed, shift=0.25, head_gain=1.0):
    """oracle glorot weights made asymmetric (`shift`), with non-trivial BatchNorm statistics (lite: pointwise biases) and one
    negative gamma; `head_gain` scales the head kernel, whose column sums are zero"""
    lite = kind == "simple_cnn_lite"
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
    ws[10 if lite else 6][2] = -0.7                     # batch_normalization_1/gamma[2] < 0
    ws[-2] = (ws[-2] - ws[-2].mean(0)) * head_gain
    om.set_weights([np.asarray(w, np.float32).astype(np.float64) for w in ws])     # the device's float32 weights, exactly
    return om


def quant_features(n, seed, scale):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, 30, 20)) + 0.5 * rng.standard_normal((n, 1, 20))).astype(np.float32)


# channels of every layer with a special role in the edge models
NEG_GAMMA = (0, 8, 10)          # gamma < 0: a decreasing epilogue (M < 0), requantized before the 2 x 2 max
ZERO_COL = 3                    # an all-zero weight column (s_w = 1)
GAMMA0 = (4, 6, 7)              # gamma = 0 (M = 0) with a mid-range, a saturating (codes 127) and a negative (codes 0) beta
GAMMA0_BETA = (0.4, 40.0, -40.0)
BQ_CH = (12, 13)                # lite: pointwise bias at +-2^23 codes
BQ_BIAS = (3.0e4, -3.0e4)


def edge_weights(kind, C, seed):
    """a quant_weights model with every sign and degenerate-channel edge of the int8 contract in every layer"""
    lite = kind == "simple_cnn_lite"
    om = quant_weights(kind, C, seed, shift=0.05, head_gain=4.0)
    ws = om.get_weights()
    names = om.weight_list()
    for i, (li, n, t) in enumerate(names):
        layer = om.layers[li]
        if n == "gamma":
            g = ws[i]
            g[list(NEG_GAMMA)] = -np.abs(g[list(NEG_GAMMA)])
            g[list(GAMMA0)] = 0.0
            ws[i + 1][list(GAMMA0)] = GAMMA0_BETA          # beta
        elif n == "depthwise_kernel" and ws[i].shape[2] > ZERO_COL:
            ws[i][:, :, ZERO_COL, :] = 0.0
        elif n in ("kernel", "pointwise_kernel") and li != len(om.layers) - 1:
            ws[i][..., ZERO_COL] = 0.0
        elif n == "bias" and lite and isinstance(layer, mo.SeparableConv2D):
            ws[i][list(BQ_CH)] = BQ_BIAS
    ws[-2][:, ZERO_COL] = 0.0                               # a head column of zeros: the class's logit is its bias
    om.set_weights([np.asarray(w, np.float32).astype(np.float64) for w in ws])
    return om


def oracle_maxima(om, feat):
    """the maxima kws_model_calibrate[_lite] collects, from the float64 oracle"""
    lite = om.model_type == "simple_cnn_lite"
    x = feat.astype(np.float64)[..., None]
    out = [np.abs(x).max()]
    for i, l in enumerate(om.layers[:-1]):
        x = l.forward(x, False)
        if lite and i in SEP:
            out.append(np.abs(l.cache[2]).max())         # u_l: the depthwise output
        if i in (3, 7, 10, 14, 18):                      # pool 1, pool 2, stage 3's ReLU6, pool 4, Dense's ReLU6
            out.append(x.max())
    return np.array(out)
