"""Case table of the recurrent-model shape tests (tests/test_rnn_shapes_gpu.py, tests/test_rnn_shapes_host.py).

simple_gru and simple_lstm run gru_fwd_kernel / gru_bwd_kernel / lstm_fwd_kernel / lstm_bwd_kernel (one template,
csrc/kws_rnn_kernels.h, with the cells of csrc/kws_gru.h and csrc/kws_lstm.h), launched from csrc/kws_rnn.hip.  Which template runs, whether a launch has to opt in to more than 64 KiB of dynamic LDS, whether the
geometry is refused and which head chain follows are all plain arithmetic on (T, F, C); that arithmetic is restated below, and the
table holds one case per branch it can take, per edge of the sequence and batch loops, and per option of the train step.  Everything
here is host-only (numpy and the float64 oracle): inputs, weights, references and the comparison that both test files apply.

The comparison is the project's existing one (tests/test_model_gpu.py: test_gru_train_forward_backward) plus a per-row bound on the
input kernel's gradient: the features carry an MFCC-like c0 column about ten times larger than the others, so a bound relative to the
tensor's largest entry is set by row 0 and hides every other feature row, the rows at the `f < F` tail of a dW tile included."""
import collections

import numpy as np

from oracle import model_oracle as mo

KINDS = ("simple_gru", "simple_lstm")

# ---- the launch arithmetic of csrc/kws_rnn_kernels.h and csrc/kws_rnn.hip, restated ---------------------------------------------
UNITS = 48                       # kGruU
HS, GS, PS = 50, 210, 50         # kGruHS, kGruGS, kGruPS: LDS row strides of the state, gate-gradient and pre-activation tiles
LDS_DEFAULT = 64 * 1024          # above this a launch calls hipFuncSetAttribute(MaxDynamicSharedMemorySize)
LDS_LIMIT = 160 * 1024           # above this the geometry is refused with KWS_ERR_UNSUPPORTED
MAX_F = 64                       # kws_model_create refuses wider recurrent models
HEAD_K = 48                      # the head's input width on the recurrent chain
ERR_UNSUPPORTED = -2             # include/kws.h


def gru_xstride(T, F):
    """floats per clip of the staged feature tile: T * F rounded up to 18 mod 32"""
    s = T * F
    while s % 32 != 18:
        s += 1
    return s


def gru_fwd_smem(T, F):
    """dynamic LDS bytes of gru_fwd_kernel and lstm_fwd_kernel: x tile, two state tiles, four pre-activation planes"""
    return 4 * (16 * gru_xstride(T, F) + 2 * 16 * HS + 4 * 16 * PS)


def gru_bwd_smem(T, F):
    """dynamic LDS bytes of gru_bwd_kernel and lstm_bwd_kernel: x tile, gate gradients, h_prev, two dh tiles"""
    return 4 * (16 * gru_xstride(T, F) + 16 * GS + 16 * HS + 2 * 16 * HS)


def kx_for(F):
    """dispatch_fwd / dispatch_bwd: the template's count of 4-feature MFMA steps"""
    kx = (F + 3) // 4
    return 5 if kx <= 5 else 10 if kx <= 10 else 16


def head_bwd_fuses(C):
    """head_bwd_fuses(m) with head_K = 48: the MFMA head, which lets the recurrent forward kernel clear the gradients"""
    return HEAD_K % 16 == 0 and HEAD_K <= 128 and C <= 48


def fwd_opts_in(T, F):
    return gru_fwd_smem(T, F) > LDS_DEFAULT


def bwd_opts_in(T, F):
    return gru_bwd_smem(T, F) > LDS_DEFAULT


def infer_supported(T, F):
    return F <= MAX_F and gru_fwd_smem(T, F) <= LDS_LIMIT


def train_supported(T, F):
    return infer_supported(T, F) and gru_bwd_smem(T, F) <= LDS_LIMIT


def branch(case):
    """(KX, forward opts in, backward opts in, head fused) of a case"""
    return kx_for(case.F), fwd_opts_in(case.T, case.F), bwd_opts_in(case.T, case.F), head_bwd_fuses(case.C)


# every combination the table is there to run, for each kind
REQUIRED_BRANCHES = {
    (5, False, False, True), (10, False, False, True), (16, False, False, True),      # width edges
    (5, False, True, True),                                                           # 34 x 20: only the backward kernel opts in
    (5, True, True, True), (10, True, True, True), (16, True, True, True),            # both opt in, every template
    (5, False, False, False),                                                         # C = 49: head forward, memset, head backward
}

# ---- the table --------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "label kind T F B C class_weights dropout_seed")

WIDE_SEED = 0x1234ABCD5678       # above 2^32: the `shi` half of the seed is not zero
REFUSED_INFER = (113, 20)        # XS = 2290: not even the forward tile fits
REFUSED_TRAIN = (110, 20)        # XS = 2226: the forward tile fits, the backward tile does not
SHRINK = (33, 1)                 # a train step at the first batch, then one at the second on the same model and workspace
SATURATED_B = 17


def _weights(C):
    return tuple([0.3] + [0.7 / (C - 1)] * (C - 1))


def _cases():
    cases = []
    for kind in KINDS:
        k = kind[len("simple_"):]

        def add(label, T, F, B, C=6, cw=None, seed=None):
            cases.append(Case("%s-%s" % (k, label), kind, T, F, B, C, cw, 4242 + T if seed is None else seed))
        # width edges: both sides of each KX switch, F % 4 != 0 and F % 16 != 0 in every template, the smallest and largest width;
        # two blocks with a tail of 5 clips
        for F in (1, 3, 20, 21, 37, 40, 41, 63, 64):
            add("width%d" % F, 9, F, 21)
        # LDS edges: under 64 KiB, backward only above, both above, the longest sequence the backward kernel accepts per template
        for T, F in ((30, 20), (34, 20), (40, 20), (109, 20), (54, 40), (34, 64)):
            add("lds%dx%d" % (T, F), T, F, 17)
        # sequence edges: the look-ahead of the saved values clamps on its first use, dU is exactly zero at T = 1
        for T in (1, 2):
            add("steps%d" % T, T, 20, 17)
        # batch edges: one block with 15 padded clips, a tile less one, a tile plus one, seven blocks with a tail of 4
        for B in (1, 15, 17, 100):
            add("batch%d" % B, 30, 20, B)
        # head variants: the smallest, the last fused and the first unfused class count
        for C in (2, 48, 49):
            add("classes%d" % C, 30, 20, 17, C=C)
        # options of the step
        add("weighted", 30, 20, 17, cw=_weights(6))
        add("seed_wide", 30, 20, 17, seed=WIDE_SEED)
        add("seed0", 30, 20, 17, seed=0)
    return cases


CASES = _cases()
# Feature seeds, moved on the float64 oracle alone: a case keeps salt 0 unless one of its clips has its two best classes within twice
# the probability tolerance, at inference or in the training pass (tests/test_rnn_shapes_host.py states the condition); then it takes
# the first salt that leaves every clip twice that margin.  No seed was chosen by looking at device output.
INPUT_SALT = {"lstm-width20": 1, "lstm-width40": 1, "lstm-lds109x20": 1, "lstm-steps1": 1, "lstm-batch15": 1, "lstm-batch100": 1,
              "lstm-classes48": 10, "lstm-classes49": 5, "lstm-seed_wide": 1}
CASE = {c.label: c for c in CASES}

# ---- tolerances: those of tests/test_model_gpu.py (test_gru_train_forward_backward), unchanged for every shape -----------
PROB_ATOL = 1e-4
LOSS_ATOL = 1e-4
GRAD_RTOL = 2e-4                 # max |got - want| < GRAD_RTOL * max |want| per tensor
ROW_FLOOR = 1e-3                 # a row of the input kernel's gradient is held to GRAD_RTOL of its own largest entry, but to no less than
                                 # ROW_FLOOR of the tensor's largest
HOST_MARGIN = 50                 # the float32 restatement of the oracle has to be this many times inside each of them


# ---- builders ---------------------------------------------------------------------------------------------------------
def saturate(om):
    """a third of the units get a gate pre-activation near +100 and another third near -100, the rest stay where they are:
    the z gate of the GRU (both bias rows, 50 each), the f and o gates of the LSTM"""
    rec = om.layers[0]
    b = np.array(rec.bias)
    u = rec.u
    if om.model_type == "simple_gru":
        b[:, 0:u // 3] = 50.0
        b[:, u // 3:2 * (u // 3)] = -50.0
    else:
        for g in (1, 3):
            b[g * u:g * u + u // 3] = 100.0
            b[g * u + u // 3:g * u + 2 * (u // 3)] = -100.0
    rec.bias = b
    return om


def oracle_model(case, dtype=np.float64, saturated=False):
    """Keras-default initialisation with every bias moved off its initial value (tests/test_model_gpu.py:
    test_other_geometries_train_and_infer), rounded to the float32 values the device holds"""
    om = mo.Model(case.kind, case.C, n_features=case.T, feature_size=case.F).init_weights(case.T + case.F)
    rng = np.random.default_rng(case.T * 1000 + case.F * 10 + case.C)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n == "bias":
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    om.set_weights(ws)
    if saturated:
        saturate(om)
    out = mo.Model(case.kind, case.C, n_features=case.T, feature_size=case.F, dtype=dtype)
    out.set_weights([w.astype(np.float32) for w in om.get_weights()])
    return out


def inputs(case):
    """(features float32 (B, T, F), labels int64 (B,), class weights float64 (C,) or None): MFCC-like features with a large negative
    c0 column"""
    rng = np.random.default_rng(case.T * 100 + case.F + 7 * case.B + 100000 * INPUT_SALT.get(case.label, 0))
    x = rng.standard_normal((case.B, case.T, case.F)) * 2.0
    x[..., 0] -= 10.0
    y = rng.integers(0, case.C, case.B)
    cw = None if case.class_weights is None else np.array(case.class_weights)
    return x.astype(np.float32), y, cw


Result = collections.namedtuple("Result", "weights infer_probs loss correct probs grads names")


def run_oracle(case, dtype=np.float64, saturated=False):
    """inference and one training pass of the oracle in `dtype`.  The dropout mask is handed over in `dtype` (0 or 1.25, exact in
    both), so that a float32 pass stays float32 throughout."""
    om = oracle_model(case, dtype, saturated)
    x, y, cw = inputs(case)
    x = x.astype(dtype)
    mask = None
    if case.dropout_seed:
        mask = (mo.dropout_keep(case.dropout_seed, case.B * case.F, 0.2).reshape(case.B, case.F) / 0.8).astype(dtype)
    with np.errstate(over="ignore"):             # e^100 in float32 is inf, and 1 / (1 + inf) is the 0 the saturated cases are about
        infer_probs = om.predict(x)
        loss, acc, probs = mo.train_forward_backward(om, x, y, None if cw is None else cw.astype(dtype), dropout_mask=mask)
    names = ["%d/%s" % (li, n) for li, n, t in om.weight_list() if t]
    return Result(om.get_weights(), infer_probs, loss, int(round(acc * case.B)), probs, [np.array(g) for g in om.grad_list()], names)


_REFERENCES = {}


def reference(case, saturated=False):
    """the float64 oracle's result for a case, computed once and shared by the tests that need it"""
    key = (case, saturated)
    if key not in _REFERENCES:
        _REFERENCES[key] = run_oracle(case, np.float64, saturated)
    return _REFERENCES[key]


def shrink_case(kind):
    return Case("%s-shrink" % kind[len("simple_"):], kind, 30, 20, SHRINK[1], 6, None, 4242 + 30)


def shrink_first_case(kind):
    return Case("%s-shrink-first" % kind[len("simple_"):], kind, 30, 20, SHRINK[0], 6, None, 4242 + 31)


def refused_train_case(kind):
    """REFUSED_TRAIN as a case: the oracle has no such limit, and inference is compared with it"""
    T, F = REFUSED_TRAIN
    return Case("%s-refused" % kind[len("simple_"):], kind, T, F, 17, 6, None, 4242 + T)


def saturated_case(kind):
    return Case("%s-saturated" % kind[len("simple_"):], kind, 30, 20, SATURATED_B, 6, None, 4242 + 30)


# ---- the comparison ---------------------------------------------------------------------------------------------------
def rel_err(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def row_errs(got, want):
    """per row f of the input kernel's gradient: max |got_f - want_f| / max(max |want_f|, ROW_FLOOR * max |want|)"""
    scale = np.maximum(np.abs(want).max(axis=1), ROW_FLOOR * np.abs(want).max())
    return np.abs(got - want).max(axis=1) / scale


def compare(ref, infer_probs, probs, loss, correct, grads, margin=1):
    """-> (figures, complaints): every figure of the comparison and the list of bounds missed, each bound divided by `margin`.
    infer_probs may be None (the second step of the shrinking-batch test runs no inference)."""
    fig, bad = collections.OrderedDict(), []

    def hold(name, value, bound):
        fig[name] = value
        if not value <= bound / margin:
            bad.append("%s: %.3g > %.3g" % (name, value, bound / margin))
    if infer_probs is not None:
        hold("infer probs", float(np.abs(infer_probs - ref.infer_probs).max()), PROB_ATOL)
        if not np.array_equal(infer_probs.argmax(-1), ref.infer_probs.argmax(-1)):
            bad.append("inference argmax differs")
    hold("train probs", float(np.abs(probs - ref.probs).max()), PROB_ATOL)
    hold("loss", abs(float(loss) - ref.loss), LOSS_ATOL)
    if int(correct) != ref.correct:
        bad.append("correct predictions: %d, oracle %d" % (int(correct), ref.correct))
    for name, g, want in zip(ref.names, grads, ref.grads):
        if g.shape != want.shape or not np.isfinite(g).all():
            bad.append("gradient of %s: wrong shape or not finite" % name)
            continue
        if not want.any():
            # exactly zero by construction (the recurrent kernel at T = 1: h_prev is the zero initial state)
            fig["grad %s (exact zero)" % name] = float(np.abs(g).max())
            if g.any():
                bad.append("gradient of %s must be exactly zero, largest entry %g" % (name, np.abs(g).max()))
            continue
        e = rel_err(g, want)
        fig["grad %s" % name] = e
        if not e < GRAD_RTOL / margin:
            bad.append("gradient of %s: rel err %.3g >= %.3g" % (name, e, GRAD_RTOL / margin))
    rows = row_errs(grads[0], ref.grads[0])
    f = int(rows.argmax())
    fig["grad 0/kernel worst row (%d)" % f] = float(rows[f])
    if not rows[f] <= GRAD_RTOL / margin:
        bad.append("row %d of the input kernel's gradient: %.3g > %.3g of its scale" % (f, rows[f], GRAD_RTOL / margin))
    return fig, bad
