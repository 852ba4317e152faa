"""Case table of the simple_cnn_lite train-step tests (tests/test_lite_train_gpu.py, tests/test_lite_train_host.py).

The train step of simple_cnn_lite (LiteCtx::forward(training = true) and LiteCtx::backward, csrc/kws_model.hip) is the only user of
dwconv_fwd / dgrad / wgrad_kernel, pw1_fwd / bwd_kernel<16>, partial_finalize_kernel and the 1x1 instantiations of conv_gemm,
conv_wgrad and conv_dgrad.  Its grids are plain arithmetic on (B, H, W): the block count and rows per block of the channel reductions
(stat_grid, capped at kStatStride = 1024 blocks), the 16-row tiles per wave of the pointwise data gradients (launch_dgrad's MW), the
side of the stride-2 'same' padding of depthwise 3, the pool windows that leave pixels out.  That arithmetic is restated below and the
table holds one case per branch it can take; REQUIRED lists those branches and tests/test_lite_train_host.py holds the table to it.
Everything here is host-only (numpy, the float64 oracle, oracle/torch_ref.py): inputs, weights, references and the comparison.

Inputs.  Stage 1 of the model (a one-channel depthwise conv, a pointwise conv, BatchNorm) does not depend on the scale of its kernels,
so with the suite's MFCC-like features (sigma 3, c0 - 10) the gradients of stage 1's depthwise and pointwise kernels are near-cancelling
sums over all B * 600 pixels, and a float32 implementation drifts from float64 there as B grows: oracle/torch_ref.py in float32 was
measured 2.95e-4 of the tensor's largest entry off at B = 220 and 6.8e-4 at B = 438 (separable_conv2d/pointwise_kernel), against a
bound of 3e-4.  With the same features times SCALE = 0.1 the stage-1 variance is comparable with BatchNorm's epsilon and the
cancellation goes away.  The condition that makes a case usable is stated on the host alone (tests/test_lite_train_host.py): the float32
restatement stays within COND_REL = 1e-4 of every gradient tensor's largest entry -- a third of the device's bound -- and within
ZERO_FLOOR on the two biases whose true gradient is zero; the unscaled features at cap2 do not meet it.

The restatement's figure is not a number of the inputs alone: torch cuts its float32 sums (BatchNorm's statistics above all) into one
chunk per intra-op thread, so the thread count is part of the arithmetic.  At B = 437, measured over a dozen seeds: with 1 or 2 threads
the sums run almost sequentially and the restatement is 4e-3 .. 2e-2 off even on the scaled features; with 4 threads it still resolves
a hard decision (next paragraph) the other way for most seeds; from 8 threads on it is within 2e-5; and the drift on the UNSCALED
features shrinks with the chunks, 1.6e-4 .. 2.6e-3 at 8 threads and below 1e-4 for most seeds at 32.  restatement_grads therefore pins
the thread count, and the condition is held at every count of RESTATEMENT_THREADS = (8, 16).  (The device keeps these sums in double.)

Hard decisions.  The backward pass routes gradients through ReLU6 gates, the ReLU of separable convolutions 3 and 4 and the pools'
arg-max (tests/tie_aware.py).  A pass of B = 437 clips holds about 1e7 of them, the closest one typically 8e-8 of its layer's
spread from its threshold, and a float32 implementation that resolves ONE the other way moves a bias-like gradient by 1e-3 .. 1e-2 of
its largest entry: with seeds taken blindly the float32 restatement itself missed the condition in four of eight large batches, each
time in the tensors below one rerouted element.  The seeds are therefore also held to nearest_decision >= TIE_MARGIN = 5e-7, about
four float32 roundings of a value the size of the layer's spread (one seed in seventy at B = 437; the 1e-6 that
cnn_path_cases.tie_eps lists to is one seed in about 2e4 there).  Every seed was chosen from these host quantities alone -- the
oracle's margins first, then the restatement's figures -- never by looking at device output.

The restatement's worst gradient figure per case (error / largest entry of the tensor, float32 torch on the host, the larger of the
figures at 8 and 16 threads):
  b1 1.2e-6, b2 1.0e-6, b3 2.0e-6, mw2 3.5e-6, under 7.8e-6, cap1 7.4e-6, mw4 9.2e-6, under2 1.2e-5, cap2 9.2e-6, small1 4.2e-6,
  small5 2.2e-6, pad00 1.4e-6, pad01 1.4e-6, pad10 9.6e-7, odd0 2.1e-6, wide 2.0e-6, weighted 3.4e-6, seed0 4.4e-6, wideseed 2.3e-6,
  c2 3.1e-6, c49 3.7e-6, shrink 8.9e-6 then 2.1e-6; 1.2e-5 overall, at under2.  Zero-gradient biases: at most 2.2e-5 (wideseed).
  cap2 with the unscaled features: 3.7e-4 at 8 threads, 3.8e-4 at 16 (separable_conv2d/pointwise_kernel), beyond COND_REL.
The device's worst gradient figure per case, measured on an MI355X (same quantity; the bound is 3e-4):
  b1 1.1e-6, b2 1.0e-6, b3 1.2e-6, mw2 9.3e-7, under 2.0e-6, cap1 2.2e-6, mw4 4.7e-6, under2 6.4e-6, cap2 7.0e-6, small1 3.0e-6,
  small5 1.6e-6, pad00 1.3e-6, pad01 2.1e-6, pad10 1.2e-6, odd0 1.8e-6, wide 1.2e-6, weighted 1.6e-6, seed0 1.3e-6, wideseed 1.6e-6,
  c2 1.2e-6, c49 8.2e-7, shrink 4.6e-6 then 1.5e-6; 7.0e-6 overall, at cap2; deterministic mode cap1 1.2e-5, b3 1.2e-6, pad01 2.1e-6.
  Zero-gradient biases: at most 8.3e-6 (wideseed); probabilities within 1.4e-6, the loss within 2.0e-6, moving statistics within a
  hundredth of their bound.

Out of scope: the remaining caps need batches whose float64 oracle step alone takes several seconds, and at which the float32
restatement itself is 1e-3 to 2e-2 off, so that the input condition cannot be checked -- the depthwise weight gradient of stage 2
(B >= 874), the stage-3 statistics (B >= 2731), the depthwise weight gradient of stage 1 (B >= 3496).  They run the same stat_grid and
the same form of row loop that cap1 and cap2 cover.  ignore_index, grad_scale and the loss clip are tests/test_loss_options_gpu.py's;
fp16 and int8 inference and graph capture have their own files."""
import collections

import numpy as np

import head_cases as hc
from cnn_path_cases import MI355X_CUS, dims                    # CnnDims of kws_model_create, shared by both CNN kinds
from oracle import model_oracle as mo

KIND = "simple_cnn_lite"
SCALE = 0.1                        # of the MFCC-like features (module docstring)
STAT_STRIDE = 1024                 # kStatStride (csrc/kws_layers.h)
CHANNELS = (16, 32, 64, 128)       # kCh[1..4]: output channels of the four stages
DW_CHANNELS = (1, 16, 32, 64)      # kCh[0..3]: channels of the depthwise kernels
DEFAULT_CLASSES = 6

# the project's bounds for these quantities (tests/test_model_gpu.py: test_lite_train_forward_backward, test_other_geometries_train_and_infer)
TOL_PROBS, TOL_LOSS = 1e-4, 1e-4
STATE_RTOL, STATE_ATOL = 2e-5, 1e-6
GRAD_REL = 3e-4                    # of the tensor's largest entry
ZERO_FLOOR = 3e-5                  # absolute, only where the true gradient is zero (test_other_geometries_train_and_infer)
COND_REL = 1e-4                    # the float32 restatement on the host: a third of GRAD_REL
RESTATEMENT_THREADS = (8, 16)      # torch intra-op thread counts at which the restatement is held to COND_REL (module docstring)
TIE_MARGIN = 5e-7                  # no hard decision of the oracle's pass closer to its threshold than this (module docstring)
PAD_MUTATION, CAP_MUTATION = 100, 10          # what a wrong padding side / a dropped last block must move, in tolerances


# ---- the launch arithmetic of csrc/kws_cnn_shape.h, restated -----------------------------------------------------------------
def stat_grid(M, C):
    """stat_grid (csrc/kws_cnn_shape.h): (blocks, rows per block) of an (M x C) channel reduction, at most STAT_STRIDE blocks"""
    R = 256 // C
    want = (M + R * 8 - 1) // (R * 8)
    nblk = min(STAT_STRIDE, max(1, want))
    rows = (M + nblk - 1) // nblk
    return (M + rows - 1) // rows, rows


def stat_capped(M, C):
    """whether stat_grid's block count hits the cap, so that a block's row loop runs past its 8 * (256 / C) rows"""
    R = 256 // C
    return (M + R * 8 - 1) // (R * 8) > STAT_STRIDE


def dgrad_mw(rows, cus):
    """the loop of dgrad_plan (csrc/kws_cnn_shape.h) for one parity class: from mw = 4 down to 1, the strictly smaller
    ceil(waves / (4 cus)) * mw is kept"""
    simds = 4 * cus
    best, best_cost = 4, -1
    for mw in (4, 3, 2, 1):
        waves = ((rows + 15) // 16 + mw - 1) // mw
        cost = ((waves + simds - 1) // simds) * mw
        if best_cost < 0 or cost < best_cost:
            best, best_cost = mw, cost
    return best


def same_pad_before(n, k, s):
    """same_pad_before (csrc/kws_cnn_shape.h): TF 'SAME' puts the odd padding pixel at the end"""
    out = -(-n // s)
    return max((out - 1) * s + k - n, 0) // 2


def stage_rows(B, nf, fs):
    """M of the four stages (CnnStep::pixels over cnn_stage's output maps): B * (H0 W0, H1 W1, H3 W3, H3 W3)"""
    d = dims(nf, fs)
    return (B * d["H0"] * d["W0"], B * d["H1"] * d["W1"], B * d["H3"] * d["W3"], B * d["H3"] * d["W3"])


def step_stat_grids(B, nf, fs):
    """every (M, C) that a train step hands to stat_grid: per stage the BatchNorm statistics / bias sums over the stage's channels and
    the depthwise weight gradient over the depthwise channels, then the Dense bias (CnnStep::dense_bias_grad: stat_grid(B, 128))"""
    out = []
    for M, C, Cin in zip(stage_rows(B, nf, fs), CHANNELS, DW_CHANNELS):
        out += [(M, C), (M, Cin)]
    return out + [(B, 128)]


def pad3(nf, fs):
    """(pt, pl) of depthwise 3, the stride-2 'same' convolution over a2"""
    d = dims(nf, fs)
    return same_pad_before(d["H2"], 3, 2), same_pad_before(d["W2"], 3, 2)


def pool_drops(nf, fs):
    """the stages (1, 2, 4) whose 2x2 'valid' pool leaves a row or a column of its input outside every window"""
    d = dims(nf, fs)
    return tuple(stage for stage, h, w in ((1, d["H0"], d["W0"]), (2, d["H1"], d["W1"]), (4, d["H3"], d["W3"])) if h % 2 or w % 2)


def branches(B, nf, fs, cus=MI355X_CUS):
    """the branches of REQUIRED that a step of B clips on an nf x fs map runs"""
    M = stage_rows(B, nf, fs)
    M_next = stage_rows(B + 1, nf, fs)
    got = {"mw%d" % dgrad_mw(M[1], cus), "pad%d%d" % pad3(nf, fs)}
    got |= {"drop%d" % stage for stage in pool_drops(nf, fs)}
    for stage in (1, 2):
        C = CHANNELS[stage - 1]
        if stat_capped(M[stage - 1], C):
            got.add("cap%d" % stage)
        elif stat_capped(M_next[stage - 1], C):
            got.add("control%d" % stage)                        # one clip more and the cap is reached
    if M[2] < 16:
        got.add("subtile")                                      # less than one 16-row MFMA tile in the GEMMs of stages 3 and 4
    return got


# every branch the table is there to run
REQUIRED = {"cap1", "cap2", "control1", "control2", "mw1", "mw2", "mw3", "mw4", "pad00", "pad01", "pad10", "pad11",
            "drop1", "drop2", "drop4", "subtile"}


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# label, frames, coefficients, batch, then the stated arithmetic at MI355X_CUS compute units -- (blocks, rows per block) of the stage-1
# and stage-2 reductions, MW of stage 2's pointwise data gradient conv_dgrad<32,16>, (pt3, pl3), the stages whose pool drops pixels, the
# rows of the stage-3 / stage-4 GEMMs -- and what the case is for.  tests/test_lite_train_host.py holds every stated value against the
# restated arithmetic.  `then`: a second step of that many clips on the same model and workspace.
Case = collections.namedtuple("Case", "label nf fs B stat1 stat2 mw2 pad3 drops m3 why C seed weighted then")


def _case(label, nf, fs, B, stat1, stat2, mw2, pad, drops, m3, why, C=DEFAULT_CLASSES, seed=None, weighted=False, then=None):
    return Case(label, nf, fs, B, stat1, stat2, mw2, pad, drops, m3, why, C, 4242 + B if seed is None else seed, weighted, then)


CASES = (
    _case("b1", 30, 20, 1, (5, 120), (3, 50), 1, (1, 1), (2, 4), 12, "M = 12 in stages 3 and 4: a sub-tile GEMM, BatchNorm over 12 samples"),
    _case("b2", 30, 20, 2, (10, 120), (5, 60), 1, (1, 1), (2, 4), 24, "M = 24: one full tile and a half"),
    _case("b3", 30, 20, 3, (15, 120), (8, 57), 1, (1, 1), (2, 4), 36, "M = 36; single-block reductions in stages 3 and 4"),
    _case("mw2", 30, 20, 110, (516, 128), (258, 64), 2, (1, 1), (2, 4), 1320, "conv_dgrad<32,16> with MW = 2"),
    _case("under", 30, 20, 218, (1022, 128), (511, 64), 2, (1, 1), (2, 4), 2616, "control: want = 1022 and 511, no cap"),
    _case("cap1", 30, 20, 219, (1019, 129), (514, 64), 3, (1, 1), (2, 4), 2628, "stage-1 cap (rows 129 of 128), MW = 3"),
    _case("mw4", 30, 20, 328, (1020, 193), (769, 64), 4, (1, 1), (2, 4), 3936, "MW = 4"),
    _case("under2", 30, 20, 436, (1022, 256), (1022, 64), 4, (1, 1), (2, 4), 5232,
          "control of the stage-2 cap: want = 1022 (not in the issue's table; REQUIRED asks for a control within one clip of EACH cap)"),
    _case("cap2", 30, 20, 437, (1021, 257), (1009, 65), 1, (1, 1), (2, 4), 5244, "stage-2 cap (rows 65 of 64), MW back to 1"),
    _case("small1", 16, 16, 1, (2, 128), (1, 64), 1, (0, 0), (), 4, "M = 4 in stages 3 and 4, 1x1 Dense kernel"),
    _case("small5", 16, 16, 5, (10, 128), (5, 64), 1, (0, 0), (), 20, "M = 20, 1x1 Dense kernel"),
    _case("pad00", 24, 16, 5, (15, 128), (8, 60), 1, (0, 0), (4,), 30, "(pt3, pl3) = (0, 0); H3 = 3 odd: the stage-4 pool drops a row"),
    _case("pad01", 26, 14, 5, (15, 122), (8, 57), 1, (0, 1), (2, 4), 30, "(0, 1); H1 = 13 and W1 = 7 odd: the stage-2 pool drops a row and a column"),
    _case("pad10", 22, 18, 5, (16, 124), (8, 62), 1, (1, 0), (2, 4), 30, "(1, 0); H1 = 11 and W1 = 9 odd"),
    _case("odd0", 31, 21, 5, (26, 126), (12, 63), 1, (1, 1), (1, 2, 4), 60, "H0 = 31 and W0 = 21 odd: the stage-1 pool drops pixels"),
    _case("wide", 24, 30, 5, (29, 125), (15, 60), 1, (0, 1), (2, 4), 60, "W > H"),
    _case("weighted", 30, 20, 33, (155, 128), (78, 64), 1, (1, 1), (2, 4), 396, "class weights [0.3] + [0.7 / 5] * 5", weighted=True),
    _case("seed0", 30, 20, 33, (155, 128), (78, 64), 1, (1, 1), (2, 4), 396, "dropout_seed = 0: no dropout", seed=0),
    _case("wideseed", 30, 20, 33, (155, 128), (78, 64), 1, (1, 1), (2, 4), 396, "a dropout seed with a non-zero high half", seed=0x1234ABCD5678),
    _case("c2", 30, 20, 33, (155, 128), (78, 64), 1, (1, 1), (2, 4), 396, "2 classes", C=2),
    _case("c49", 30, 20, 33, (155, 128), (78, 64), 1, (1, 1), (2, 4), 396, "49 classes: the head is not fused", C=49),
    _case("shrink", 30, 20, 219, (1019, 129), (514, 64), 3, (1, 1), (2, 4), 2628,
          "219 clips, then 3 on the same model and workspace: the second step must not read the first's partial sums beyond its own nblk", then=3),
)
CASE = {c.label: c for c in CASES}
DETERMINISTIC = ("cap1", "b3", "pad01")       # run once more with set_deterministic(True)

# seeds of the weights (s), the perturbation (s + 1), the features (s + 2) and the labels (s + 3) of a case: chosen on the host
# quantities of tests/test_lite_train_host.py alone (module docstring)
# the small batches: of a hundred seeds each the one with the largest nearest_decision
SEED = dict(b1=8015, b2=8121, b3=8282, small1=8993, small5=9074, pad00=9156, pad01=9254, pad10=9399, odd0=9417, wide=9532,
            weighted=9624, seed0=9731, wideseed=9844, c2=9925, c49=10017)
# the large batches: of a few hundred seeds each (cap2: 1920, 23 of them at or above TIE_MARGIN) the one with the largest
# nearest_decision that also meets the restatement's condition, measured at 4, 8, 16 and 32 threads (at mw4's largest margin, 9.5e-7,
# the restatement resolves a decision the other way at 8 threads and is 9e-3 off).  cap2: the one whose scaled features meet the
# condition at 8, 16 and 32 threads while its unscaled features miss it by about the same 3.7e-4 .. 4.8e-4 at each of them
# (a drift; at most other seeds the unscaled figure is one rerouted element at some thread count and within 1e-4 at another)
SEED.update(mw2=6077, under=4024, cap1=3134, mw4=2277, under2=1132, cap2=1057, shrink=5178)


def batches(case):
    return (case.B,) if case.then is None else (case.B, case.then)


def dropout_seed(case, B):
    return case.seed if B == case.B else 4242 + B


# ---- builders ----------------------------------------------------------------------------------------------------------------
def weights(case):
    """Keras-order weights: init_weights and the gamma / beta / bias / moving-statistic perturbation of tests/test_model_gpu.py:
    build(), rounded to float32 once -- the oracle and the device get these values"""
    s = SEED[case.label]
    om = mo.Model(KIND, case.C, n_features=case.nf, feature_size=case.fs).init_weights(s)
    rng = np.random.default_rng(s + 1)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    return [np.asarray(w, np.float32) for w in ws]


def oracle_model(case, ws):
    om = mo.Model(KIND, case.C, n_features=case.nf, feature_size=case.fs)
    om.set_weights([w.astype(np.float64) for w in ws])
    return om


def inputs(case, B, scale=SCALE):
    """(features float32 (B, nf, fs), labels int64 (B,), class weights float64 (C,) or None): scale times the MFCC-like features of
    tests/test_model_gpu.py (head_cases.features draws the same values on any map)"""
    s = SEED[case.label] + (0 if B == case.B else 5)
    x = (np.float32(scale) * hc.features(B, s + 2, case.nf, case.fs)).astype(np.float32)
    y = np.random.default_rng(s + 3).integers(0, case.C, B)
    cw = np.array([0.3] + [0.7 / (case.C - 1)] * (case.C - 1)) if case.weighted else None
    return x, y, cw


def nearest_decision(om):
    """after a training forward of the oracle: how close the closest hard decision of the pass sits to its threshold -- a ReLU6 gate
    (y against 0 and 6), the ReLU of separable convolutions 3 and 4, the gap between the two largest elements of a pool window where
    they differ -- relative to the standard deviation of the layer's input, as tests/tie_aware.py measures it"""
    best, y = np.inf, None
    for l in om.layers:
        if isinstance(l, mo.SeparableConv2D) and l.relu:
            pre = l.cache[2] @ l.pointwise_kernel.reshape(l.cin, l.cout) + l.bias
            best = min(best, float(np.abs(pre).min() / pre.std()))
        elif isinstance(l, mo.BatchNorm):
            y = l.cache[0] * l.gamma + l.beta
        elif isinstance(l, mo.Dense):
            y = l.x @ l.kernel + l.bias
        elif isinstance(l, mo.ReLU6):
            best = min(best, float(min(np.abs(y).min(), np.abs(y - 6.0).min()) / y.std()))
            y = np.minimum(np.maximum(y, 0), 6)
        elif isinstance(l, mo.MaxPool2):
            Ho, Wo = y.shape[1] // 2, y.shape[2] // 2
            win = np.sort(np.stack([y[:, 0:2 * Ho:2, 0:2 * Wo:2], y[:, 0:2 * Ho:2, 1:2 * Wo:2], y[:, 1:2 * Ho:2, 0:2 * Wo:2],
                                    y[:, 1:2 * Ho:2, 1:2 * Wo:2]], 0), axis=0)
            gap = win[3] - win[2]
            if (gap > 0).any():
                best = min(best, float(gap[gap > 0].min() / y.std()))
            y = win[3]
    return best


# one train step of the oracle: its inputs, the float64 results that the device is compared with, and nearest_decision of the pass
Step = collections.namedtuple("Step", "B x y cw seed probs loss correct grads weights margin")
Reference = collections.namedtuple("Reference", "weights0 names trainable zero_grad steps")
_REFERENCES = {}


def reference(case, scale=SCALE):
    """the oracle's results for a case, computed once per (case, scale): the start weights (float32), the tensor names, and per step the
    probabilities, mean loss, correct count, gradients and the weights after it (the moving statistics changed)"""
    key = (case.label, scale)
    if key not in _REFERENCES:
        ws = weights(case)
        om = oracle_model(case, ws)
        wl = om.weight_list()
        steps = []
        for B in batches(case):
            x, y, cw = inputs(case, B, scale)
            seed = dropout_seed(case, B)
            loss, acc, p = mo.train_forward_backward(om, x.astype(np.float64), y, cw, dropout_seed=seed or None)
            step = Step(B, x, y, cw, seed, p, loss, int(round(acc * B)), [np.array(g) for g in om.grad_list()], om.get_weights(),
                        nearest_decision(om))
            for a in (x, y, p) + tuple(step.grads) + tuple(step.weights):
                a.setflags(write=False)
            steps.append(step)
        # a pointwise bias straight in front of a BatchNorm (no ReLU in between: stages 1 and 2) has a zero gradient
        zero = ["%d/%s" % (li, n) for li, n, _ in wl if n == "bias" and isinstance(om.layers[li], mo.SeparableConv2D) and not om.layers[li].relu]
        _REFERENCES[key] = Reference(ws, ["%d/%s" % (li, n) for li, n, _ in wl], [t for _, _, t in wl], zero, tuple(steps))
    return _REFERENCES[key]


# ---- the comparison ------------------------------------------------------------------------------------------------------------
# err and bound are in the quantity's own units (moving statistics: |got - want| over atol + rtol |want|, bound 1); rel = err over the
# largest entry of the oracle's tensor, the figure that the docstrings quote
Figure = collections.namedtuple("Figure", "name err bound rel")


def grad_figures(ref, step, grads, rel=GRAD_REL, floor=ZERO_FLOOR):
    """each gradient tensor within rel * max |want|; the absolute floor only where the true gradient is zero"""
    names = [n for n, t in zip(ref.names, ref.trainable) if t]
    assert len(grads) == len(step.grads) == len(names)
    figs = []
    for name, g, want in zip(names, grads, step.grads):
        g = np.asarray(g, np.float64)
        assert g.shape == want.shape, (name, g.shape, want.shape)
        err, top = float(np.abs(g - want).max()), float(np.abs(want).max())
        err = err if np.isfinite(g).all() else float("inf")
        if name in ref.zero_grad:
            assert top < 1e-12, (name, top)
            figs.append(Figure("grad " + name, err, floor, float("nan")))
        else:
            figs.append(Figure("grad " + name, err, rel * top, err / top))
    return figs


def compare(ref, step, probs, loss, correct, grads, weights_after):
    """the device's results of one step against the oracle's, by the project's existing bounds -> the figures of every quantity"""
    probs = np.asarray(probs, np.float64)
    assert probs.shape == step.probs.shape
    perr = float(np.abs(probs - step.probs).max()) if np.isfinite(probs).all() else float("inf")
    figs = [Figure("probs", perr, TOL_PROBS, perr),
            Figure("loss", abs(float(loss) - step.loss), TOL_LOSS, abs(float(loss) - step.loss) / abs(step.loss)),
            Figure("correct", abs(float(correct) - step.correct), 0.0, float("nan"))]
    for name, t, got, want in zip(ref.names, ref.trainable, weights_after, step.weights):
        if not t:
            got = np.asarray(got, np.float64)
            e = float((np.abs(got - want) / (STATE_ATOL + STATE_RTOL * np.abs(want))).max()) if np.isfinite(got).all() else float("inf")
            figs.append(Figure("state " + name, e, 1.0, float(np.abs(got - want).max() / np.abs(want).max())))
    return figs + grad_figures(ref, step, grads)


def failures(figs):
    return [f for f in figs if not f.err <= f.bound]


def worst_gradient(figs):
    """the figure the docstrings quote: the largest error of a gradient tensor relative to that tensor's largest entry"""
    return max((f for f in figs if f.name.startswith("grad ") and f.rel == f.rel), key=lambda f: f.rel)


# ---- the float32 restatement (the condition on the inputs) ---------------------------------------------------------------------
def restatement_grads(case, scale=SCALE, threads=RESTATEMENT_THREADS[0]):
    """per step, the gradients of oracle/torch_ref.py's TorchModel in float32 from the same weights, inputs and dropout mask, with
    torch's intra-op thread count pinned (module docstring: its float32 sums are cut into one chunk per thread)"""
    import torch
    from oracle import torch_ref as tr
    ref = reference(case, scale)
    flat = dims(case.nf, case.fs)["flat"]
    out = []
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        tm = tr.TorchModel(KIND, ref.weights0, ref.trainable, dtype=torch.float32)
        for st in ref.steps:
            mask = (mo.dropout_keep(st.seed, st.B * flat, 0.5) / 0.5).reshape(st.B, flat) if st.seed else None
            _, _, grads = tm.train_step(None, np.array(st.x), np.array(st.y), st.cw, mask)      # copies: the reference arrays are read-only
            out.append([g.numpy().astype(np.float64) for g in grads])
    finally:
        torch.set_num_threads(before)
    return out


# ---- what a wrong kernel would give (tests/test_lite_train_host.py: the tests can fail) --------------------------------------------
def swapped_padding_dw3_grad(case):
    """(the oracle's gradient of stage 3's depthwise kernel, the same with the odd padding pixel of every stride-2 'same' convolution
    moved to the front), as lite_map_cases.swapped_padding_probs patches the oracle"""
    ref = reference(case)
    st = ref.steps[0]
    om = oracle_model(case, ref.weights0)
    orig = mo.same_pad

    def swapped(n_in, k, s):
        n_out, before, after = orig(n_in, k, s)
        return (n_out, after, before) if s == 2 else (n_out, before, after)
    mo.same_pad = swapped
    try:
        mo.train_forward_backward(om, st.x.astype(np.float64), st.y, st.cw, dropout_seed=st.seed or None)
    finally:
        mo.same_pad = orig
    names = [n for n, t in zip(ref.names, ref.trainable) if t]
    i = names.index("8/depthwise_kernel")
    return st.grads[i], om.grad_list()[i]


def truncated_gamma1_grad(case, keep_rows):
    """(the oracle's gradient of stage 1's BatchNorm gamma, the same summed over the first keep_rows pixel rows only): what a finalize
    kernel that misses the reduction's last blocks would leave"""
    ref = reference(case)
    st = ref.steps[0]
    om = oracle_model(case, ref.weights0)
    _, _, p = mo.train_forward_backward(om, st.x.astype(np.float64), st.y, st.cw, dropout_seed=st.seed or None)
    d = mo.loss_and_grad(p, st.y, st.cw)[1]
    for l in reversed(om.layers[2:]):
        d = l.backward(d)
    terms = (d * om.layers[1].cache[0]).reshape(-1, CHANNELS[0])
    full = terms.sum(0)
    np.testing.assert_allclose(full, om.layers[1].grads["gamma"], rtol=1e-12, atol=1e-15)
    return full, terms[:keep_rows].sum(0)
