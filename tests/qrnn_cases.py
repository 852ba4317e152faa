"""Case table of the int8 recurrent forward's shape tests (tests/test_quant_rnn_shapes_gpu.py, tests/test_quant_rnn_shapes_host.py).

qrnn_kernel<G> (csrc/kws_quant_rnn.hip) is promised for feature_size F in 1..64, T in 1..128 steps and C in 2..48 classes
(include/kws.h).  F decides which 16-byte lane quarters of the A fragment are live and how much of W's one k-step is zero padding; T
drives the one-step-ahead prefetch and the ping-pong of the LDS tile that carries h from the C to the A layout; C selects the partly
live head tiles and bounds the softmax rows; B decides the dead rows of a 16-clip wave.  The table holds one sweep per axis, the other
axes at BASE (off the default 30 x 20), and a few corners.  Everything here is host-only (numpy and tests/int8_rnn_ref.py): weights,
features, references, the tolerances and the comparison both test files apply.

Two weight designs run at every shape.  The saturated GRU (z = 0 and r = 1 exactly, h' = mx_h + mh_h) keeps the whole forward on the
exactly restated path, so the device logits must be bit-equal to the restatement's: any layout, padding or parity mistake shows.
General weights, for both kinds, leave the device's sigmoidf_ / tanh_fast_ in play; they are held to the tolerances of TOL below."""
import collections

import numpy as np

import int8_rnn_ref as ref

U = ref.U
KINDS = ("simple_gru", "simple_lstm")
BASE = (7, 33, 17)                                   # (T, F, C) of the sweeps' other axes, of the extra feature sets and of the buffers
F_SWEEP = (1, 15, 16, 17, 32, 33, 48, 49, 63, 64)    # every quarter edge of the A fragment, one live lane in a quarter, no zero padding
T_SWEEP = (1, 2, 3, 127, 128)                        # no prefetch at all, both parities of the ping-pong tile, the promised maximum
C_SWEEP = (2, 15, 16, 17, 31, 32, 33, 47, 48)        # the list of tests/test_quant_heads_gpu.py
B_SWEEP = (1, 15, 16, 17, 33)                        # one clip, a tile less one, a tile, a tile plus one, two tiles plus one
CORNERS = ((1, 1, 2), (128, 64, 48), (127, 63, 47), (2, 17, 17))
N_EXACT = 49                                         # three full tiles and one row
N_SHARE = 257                                        # sixteen tiles and one row: where a share of clips is asserted
NOISE_DRAWS = 5
EPS = float(np.finfo(np.float32).eps)

Case = collections.namedtuple("Case", "label array kind weights variant T F C B N start")
# array: the key of the model and feature array the case runs on (the B sweep shares one: its cases are the clips
#        [start, start + B) of the N-clip array, from an odd clip, so nothing is aligned to the 16-clip tile)
# weights: "saturated" or "random";  variant: "plain", or one of the extra feature sets / models of the exact part


def _shapes():
    T0, F0, C0 = BASE
    out = [(T0, F, C0) for F in F_SWEEP] + [(T, F0, C0) for T in T_SWEEP] + [(T0, F0, C) for C in C_SWEEP] + list(CORNERS)
    return list(collections.OrderedDict.fromkeys(out))


def _cases(kind, weights, N):
    k = "%s-%s" % ("sat" if weights == "saturated" else "gen", kind[len("simple_"):])
    cases = []
    for T, F, C in _shapes():
        key = "%s-%dx%dx%d" % (k, T, F, C)
        cases.append(Case(key, key, kind, weights, "plain", T, F, C, N, N, 0))
    T, F, C = BASE
    key = "%s-%dx%dx%d" % (k, T, F, C)
    for B in B_SWEEP:
        cases.append(Case("%s-b%d" % (key, B), key, kind, weights, "plain", T, F, C, B, N, 1))
    return cases


EXTRA_VARIANTS = ("zeros", "spread", "zero_bias")
EXACT_CASES = _cases("simple_gru", "saturated", N_EXACT) + [
    Case("sat-gru-%s" % v, "sat-gru-%s" % v, "simple_gru", "saturated", v, BASE[0], BASE[1], BASE[2], N_EXACT, N_EXACT, 0)
    for v in EXTRA_VARIANTS]
TOLERANCE_CASES = _cases("simple_gru", "random", N_SHARE) + _cases("simple_lstm", "random", N_SHARE)
ZERO_STEP, ZERO_CLIP, SPARSE_CLIP = 3, 5, 11         # of the "zeros" and "zero_bias" variants

# ---- tolerances of the general-weight cases ---------------------------------------------------------------------------------------
# The device's gate functions are within 1e-6 of the float64 ones (include/kws.h).  Where that moves no requantized code a logit moves
# by about T x 8 ulp of its magnitude: tight_bound().  Where v * inv lies that close to a rounding tie one code flips by one step.  How
# far that carries is measured on the restatement alone: every gate output moved by a draw uniform within +-1e-6 (ref.gate_noise),
# NOISE_DRAWS draws per array.
#   D        the largest logit deviation of a perturbed run from the unperturbed one, over all clips and draws
#   s        the smallest share of clips, over the draws, whose deviation stays inside the tight bound
#   qerr     the largest deviation of the restatement from the unquantized float64 model
#   excluded the largest share of clips, over the draws, that the arg-max rule below leaves out
# The device is one more draw and may flip a few codes where each host draw flipped one, so a device clip outside the tight bound is
# held to 3 D; 3 D < qerr (the test tells the kernel from an unquantized one), the device's clean share is at least min(0.5, s / 2),
# and its arg-max equals the restatement's wherever the top-two gap exceeds twice the bound the clip is held to: the tight bound for
# a clip inside it, 3 D for the others (at most 5 % excluded).
# How 3 D compares with qerr is a matter of the model.  One flipped code of h_T moves a logit by one step of h times a head weight of
# up to 3.5 (they are normal); the rounding of all 48 codes, which qerr sees on every clip, moves it by about 0.29 sqrt(48) = 2
# steps, at most 4 to 5 times that over an array: 3 D is about qerr, wherever the flip happens to fall.
#   LSTM: |h| <= 1, so the step of an h code does not grow with the features, while the error of the features' own codes does, and
#         reaches the gates.  At a feature scale of 30 qerr is about ten times 3 D at every shape but F = 1 (one feature: its code is
#         always +-127 and carries no error).
#   GRU:  the candidate is linear, h grows with the features, D and qerr grow together: over four seeds each at T = 7 and T = 128,
#         3 D / qerr lay mostly between 0.5 and 2.3 at every scale from 0.01 to 300 (above 1 for all twenty seeds tried at T = 127
#         with the scale 3 of the exact cases).  Scale 1 keeps s at 0.95 at T = 128 (0.82 at scale 3) and the features moving in
#         time (far below it the clips are all but constant); the feature seed does the rest.
# salt: the feature seed's offset.  An array keeps salt 0 unless 3 D >= qerr or excluded > 0.05 there, or its five draws flipped no
# code at all (D at most ten times the largest tight bound: such a D says nothing about a flip, and the first one on the device would
# break 3 D); then it takes the first salt at which none of the three holds.  The arrays of the B sweep must also keep clip `start`,
# the one clip of the B = 1 case, inside the tight bound in all five draws: the share rule asks that clip to be clean on the device.
# Every scale, figure and salt was found on the host; none was chosen by looking at device output.
# tests/test_quant_rnn_shapes_host.py recomputes every figure and fails if one drifts.
Tol = collections.namedtuple("Tol", "salt D s qerr excluded")
TOL_SCALE = {"simple_gru": 1.0, "simple_lstm": 30.0}
TOL = {
    "gen-gru-7x1x17": Tol(0, 3.554851e-02, 0.9844, 1.635561e-01, 0.0000),
    "gen-gru-7x15x17": Tol(0, 3.314257e-02, 0.9844, 1.447893e-01, 0.0039),
    "gen-gru-7x16x17": Tol(0, 2.859855e-02, 0.9922, 1.149004e-01, 0.0039),
    "gen-gru-7x17x17": Tol(1, 2.969956e-02, 0.9805, 1.171794e-01, 0.0039),
    "gen-gru-7x32x17": Tol(2, 2.754259e-02, 0.9883, 1.420840e-01, 0.0078),
    "gen-gru-7x33x17": Tol(0, 3.086567e-02, 0.9844, 1.155450e-01, 0.0039),
    "gen-gru-7x48x17": Tol(0, 3.844118e-02, 0.9728, 1.311116e-01, 0.0195),
    "gen-gru-7x49x17": Tol(0, 2.777719e-02, 0.9844, 1.281238e-01, 0.0039),
    "gen-gru-7x63x17": Tol(0, 1.969433e-02, 0.9883, 1.245354e-01, 0.0039),
    "gen-gru-7x64x17": Tol(0, 2.270794e-02, 0.9805, 1.147974e-01, 0.0000),
    "gen-gru-1x33x17": Tol(1, 1.002692e-02, 0.7043, 7.675703e-02, 0.0272),
    "gen-gru-2x33x17": Tol(0, 1.972723e-02, 0.9883, 1.266443e-01, 0.0000),
    "gen-gru-3x33x17": Tol(0, 1.972210e-02, 0.9922, 1.016408e-01, 0.0000),
    "gen-gru-127x33x17": Tol(1, 4.056263e-02, 0.9533, 1.683299e-01, 0.0078),
    "gen-gru-128x33x17": Tol(0, 4.456878e-02, 0.9611, 1.634466e-01, 0.0117),
    "gen-gru-7x33x2": Tol(0, 1.112473e-02, 0.9844, 8.385036e-02, 0.0000),
    "gen-gru-7x33x15": Tol(2, 2.322769e-02, 0.9844, 1.244138e-01, 0.0039),
    "gen-gru-7x33x16": Tol(1, 2.199340e-02, 0.9767, 1.552596e-01, 0.0039),
    "gen-gru-7x33x31": Tol(1, 3.063869e-02, 0.9805, 1.189519e-01, 0.0000),
    "gen-gru-7x33x32": Tol(0, 3.143963e-02, 0.9844, 1.082469e-01, 0.0039),
    "gen-gru-7x33x33": Tol(0, 3.322744e-02, 0.9844, 1.665216e-01, 0.0000),
    "gen-gru-7x33x47": Tol(1, 2.925873e-02, 0.9844, 1.354765e-01, 0.0039),
    "gen-gru-7x33x48": Tol(0, 2.516782e-02, 0.9767, 1.425721e-01, 0.0078),
    "gen-gru-1x1x2": Tol(0, 2.696037e-03, 0.9767, 6.868209e-02, 0.0000),
    "gen-gru-128x64x48": Tol(2, 3.956640e-02, 0.9650, 1.338826e-01, 0.0117),
    "gen-gru-127x63x47": Tol(1, 4.877651e-02, 0.9650, 1.610676e-01, 0.0117),
    "gen-gru-2x17x17": Tol(0, 2.707005e-02, 0.9844, 1.017083e-01, 0.0000),
    "gen-lstm-7x1x17": Tol(0, 2.147675e-02, 0.9844, 9.074560e-02, 0.0039),
    "gen-lstm-7x15x17": Tol(0, 1.458538e-02, 0.9922, 3.416555e-01, 0.0000),
    "gen-lstm-7x16x17": Tol(0, 1.422310e-02, 0.9922, 3.869313e-01, 0.0000),
    "gen-lstm-7x17x17": Tol(1, 1.598549e-02, 0.9922, 6.676415e-01, 0.0039),
    "gen-lstm-7x32x17": Tol(0, 2.622700e-02, 0.9961, 4.488920e-01, 0.0000),
    "gen-lstm-7x33x17": Tol(0, 2.212346e-02, 0.9883, 4.918758e-01, 0.0000),
    "gen-lstm-7x48x17": Tol(0, 2.235448e-02, 0.9767, 7.550178e-01, 0.0000),
    "gen-lstm-7x49x17": Tol(0, 1.412082e-02, 0.9883, 5.961856e-01, 0.0000),
    "gen-lstm-7x63x17": Tol(0, 1.517868e-02, 0.9922, 4.552964e-01, 0.0039),
    "gen-lstm-7x64x17": Tol(0, 2.370489e-02, 0.9922, 5.041869e-01, 0.0000),
    "gen-lstm-1x33x17": Tol(0, 1.387310e-02, 0.6498, 3.758084e-01, 0.0233),
    "gen-lstm-2x33x17": Tol(0, 1.251674e-02, 0.9767, 5.738154e-01, 0.0039),
    "gen-lstm-3x33x17": Tol(0, 1.169109e-02, 0.9922, 4.200338e-01, 0.0000),
    "gen-lstm-127x33x17": Tol(2, 1.908410e-02, 0.9883, 5.593020e-01, 0.0000),
    "gen-lstm-128x33x17": Tol(0, 2.067113e-02, 0.9883, 6.171466e-01, 0.0039),
    "gen-lstm-7x33x2": Tol(0, 1.593590e-02, 0.9883, 4.363504e-01, 0.0000),
    "gen-lstm-7x33x15": Tol(0, 2.184653e-02, 0.9805, 4.146341e-01, 0.0000),
    "gen-lstm-7x33x16": Tol(0, 1.748395e-02, 0.9922, 4.352624e-01, 0.0039),
    "gen-lstm-7x33x31": Tol(0, 2.614558e-02, 0.9922, 6.463108e-01, 0.0000),
    "gen-lstm-7x33x32": Tol(0, 1.921487e-02, 0.9883, 3.993938e-01, 0.0000),
    "gen-lstm-7x33x33": Tol(0, 1.418781e-02, 0.9922, 4.764269e-01, 0.0000),
    "gen-lstm-7x33x47": Tol(0, 1.749754e-02, 0.9922, 5.539232e-01, 0.0000),
    "gen-lstm-7x33x48": Tol(0, 2.398360e-02, 0.9883, 7.007742e-01, 0.0039),
    "gen-lstm-1x1x2": Tol(0, 4.468977e-03, 0.8366, 4.036342e-02, 0.0000),
    "gen-lstm-128x64x48": Tol(1, 1.721811e-02, 0.9961, 5.279346e-01, 0.0000),
    "gen-lstm-127x63x47": Tol(1, 1.799583e-02, 0.9883, 6.265013e-01, 0.0039),
    "gen-lstm-2x17x17": Tol(1, 1.411915e-02, 0.9728, 3.801200e-01, 0.0000),
}
DEVICE_FACTOR = 3.0
MAX_EXCLUDED = 0.05


def tight_bound(T, logits):
    """per clip: T x 8 ulp of (1 + the clip's largest |logit|), the bound of tests/test_quant_rnn_gpu.py with the case's own T"""
    return T * 8 * EPS * (1.0 + np.abs(np.asarray(logits, np.float64)).max(1))


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def _seed(case):
    return 1000 * case.T + 10 * case.F + case.C


def features(n, T, F, seed, scale=3.0):
    """_features of tests/test_quant_rnn_gpu.py at any (T, F)"""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, T, F)) + 0.5 * rng.standard_normal((n, 1, F))).astype(np.float32)


def saturated_gru(F, C, seed):
    """_linear_gru of tests/test_quant_rnn_gpu.py at any F: z-gate columns with zero weights and bias -100 (z = 0 exactly), r-gate bias
    +100 (r = 1 exactly), so h' = mx_h + mh_h, a linear recurrence entirely on the int8 path.  The input kernel is scaled by
    sqrt(20 / F), which keeps the spread of the pre-activations; U_h has a spectral radius of about 0.5, so h stays bounded for any T."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(-1.0, 1.3, (F, 3 * U)) * 0.3 * np.sqrt(20.0 / F)
    rk = rng.uniform(-1.0, 1.2, (U, 3 * U)) * 0.12
    b = rng.normal(0.0, 0.3, (2, 3 * U))
    k[:, :U] = 0.0
    rk[:, :U] = 0.0
    b[0, :U], b[1, :U] = -100.0, 0.0
    b[0, U:2 * U], b[1, U:2 * U] = 100.0, 0.0
    hk = rng.normal(0.0, 1.0, (U, C))
    hb = rng.normal(0.0, 0.3, C)
    return [np.asarray(w, np.float32) for w in (k, rk, b, hk, hb)]


def random_weights(kind, F, C, seed):
    """_random of tests/test_quant_rnn_gpu.py at any F: asymmetric weights of a trained-looking scale"""
    rng = np.random.default_rng(seed)
    G = ref.GATES[kind]
    k = rng.uniform(-1.0, 1.4, (F, G * U)) / np.sqrt(20) * 0.5 * np.sqrt(20.0 / F)
    rk = rng.uniform(-1.0, 1.2, (U, G * U)) / np.sqrt(U)
    b = rng.normal(0.0, 0.3, (2, G * U) if G == 3 else (G * U,))
    hk = rng.normal(0.0, 1.0, (U, C))
    hb = rng.normal(0.0, 0.3, C)
    return [np.asarray(w, np.float32) for w in (k, rk, b, hk, hb)]


def weights(case):
    """[kernel, recurrent_kernel, bias, head kernel, head bias] of a case (float32, the model's Keras order)"""
    if case.weights == "random":
        return random_weights(case.kind, case.F, case.C, _seed(case))
    ws = saturated_gru(case.F, case.C, _seed(case))
    if case.variant == "zero_bias":                  # no bias on the candidate columns: an all-zero clip keeps h = 0 exactly
        ws[2][:, 2 * U:] = 0.0
    if case.variant == "spread":                     # features of up to 1000 times the usual size: the r gate takes no input either,
        ws[0][:, U:2 * U] = 0.0                      # so that it stays at +100 whatever the clip's factor
        ws[1][:, U:2 * U] = 0.0
    return ws


def spread_factors(case):
    """the "spread" variant's factor of every clip: 10 ** uniform(-3, 3)"""
    return (10.0 ** np.random.default_rng(_seed(case) + 2).uniform(-3.0, 3.0, case.N)).astype(np.float32)


def feature_array(case):
    """the N clips of a case's array, float32 (N, T, F)"""
    salt = TOL[case.array].salt if case.array in TOL else 0
    x = features(case.N, case.T, case.F, _seed(case) + 1 + 100000 * salt, TOL_SCALE[case.kind] if case.weights == "random" else 3.0)
    if case.variant in ("zeros", "zero_bias"):
        x[ZERO_CLIP] = 0.0                           # a whole clip: m == 0 at every step (and, with zero_bias, for every h row)
    if case.variant == "zeros":
        x[:, ZERO_STEP] = 0.0                        # one step of every clip
        x[SPARSE_CLIP] = 0.0
        x[SPARSE_CLIP, 2, 7] = 1.5                   # a clip of zeros with a single value: one code 127 in one quarter
    if case.variant == "spread":                     # a row scale read from the wrong lane of a quarter cannot hide
        x *= spread_factors(case)[:, None, None]
    return x


def clips(case, a):
    """the case's own clips of something computed on its array"""
    return a[case.start:case.start + case.B]


_REFERENCES = {}


def reference(case):
    """(logits, probs, argmax) of the restatement on the whole array of a case, computed once per array and shared"""
    if case.array not in _REFERENCES:
        out = ref.forward(case.kind, ref.quantize(case.kind, weights(case)), feature_array(case))
        for a in out:
            a.setflags(write=False)
        _REFERENCES[case.array] = out
    return _REFERENCES[case.array]


def top2_gap(logits):
    top2 = np.sort(np.asarray(logits, np.float64), 1)[:, -2:]
    return top2[:, 1] - top2[:, 0]


def deviation(logits, want):
    """per clip: the largest |logit - restatement|"""
    return np.abs(np.asarray(logits, np.float64) - np.asarray(want, np.float64)).max(1)


def noise_deviations(case):
    """per draw of the perturbed restatement: every clip's deviation from the unperturbed run, (NOISE_DRAWS, N)"""
    arr, x = ref.quantize(case.kind, weights(case)), feature_array(case)
    wl = reference(case)[0]
    return np.stack([deviation(ref.forward(case.kind, arr, x, ref.gate_noise(7919 * (k + 1) + _seed(case)))[0], wl)
                     for k in range(NOISE_DRAWS)])


def tolerance_figures(case, devs=None):
    """Tol of a case's array, from the restatement alone (the salt is the table's); devs: noise_deviations(case), if at hand"""
    ws = weights(case)
    x = feature_array(case)
    wl = reference(case)[0]
    tight = tight_bound(case.T, wl)
    devs = noise_deviations(case) if devs is None else devs
    D = float(max(dev.max() for dev in devs))
    s = float(min((dev <= tight).mean() for dev in devs))
    qerr = float(np.abs(wl - ref.float_forward(case.kind, ws, x)).max())
    gap = top2_gap(wl)
    excluded = float(max((gap <= 2 * np.where(dev <= tight, tight, DEVICE_FACTOR * D)).mean() for dev in devs))
    return Tol(TOL[case.array].salt if case.array in TOL else 0, D, s, qerr, excluded)


def compare_tolerance(case, logits, argmax):
    """the tolerance part's rules on the case's own clips -> (figures, complaints)"""
    tol = TOL[case.array]
    wl, _, wa = (clips(case, a) for a in reference(case))
    err = deviation(logits, wl)
    tight = tight_bound(case.T, wl)
    clean = err <= tight
    loose = DEVICE_FACTOR * tol.D
    fig = collections.OrderedDict(worst=float(err.max()), clean=float(clean.mean()), D=tol.D, s=tol.s, qerr=tol.qerr)
    bad = []
    if not (err[~clean] <= loose).all():
        bad.append("%d clips outside the tight bound deviate by more than 3 D = %.3g, the worst by %.3g" %
                   ((err[~clean] > loose).sum(), loose, err.max()))
    if not clean.mean() >= min(0.5, tol.s / 2):                      # at B = 1 this asks the one clip to be inside the tight bound
        bad.append("only %.3f of the clips are inside the tight bound, %.3f asked" % (clean.mean(), min(0.5, tol.s / 2)))
    decided = top2_gap(wl) > 2 * np.where(clean, tight, loose)
    fig["decided"] = float(decided.mean())
    wrong = np.nonzero(decided & (np.asarray(argmax) != wa))[0]
    if wrong.size:
        bad.append("arg-max differs on %d decided clips, first %s" % (wrong.size, wrong[:3]))
    return fig, bad


# ---- head cases (both kinds): GRU saturated, so also bit-comparable; LSTM general ----------------------------------------------------
def head_case(kind, C, N, tag):
    sat = kind == "simple_gru"
    key = "%s-%s-%s%d" % ("sat" if sat else "gen", kind[len("simple_"):], tag, C)
    return Case(key, key, kind, "saturated" if sat else "random", "plain", BASE[0], BASE[1], C, N, N, 0)


TIE_CLASSES = (36, 48)
UNDERFLOW_C = 33
UNDERFLOW_LEAD = 110.0


def tie_pairs(C):
    """column pairs (i < j) across a tile boundary: the last lane of tile 0 and the first of tile 1; the last lane of tile 1 and the
    last live lane of tile 2 (47 at C = 48)"""
    return ((15, 16), (31, C - 1))


def tied_weights(case):
    """column j := column i (kernel and bias) for every pair, both biases raised by three times the spread of the logits (measured on
    the restatement), so that the pairs win many clips"""
    ws = weights(case)
    lg = reference(case)[0]
    boost = 3.0 * float(lg.std(0).mean())
    hk, hb = ws[3].copy(), ws[4].copy()
    for i, j in tie_pairs(case.C):
        hb[i] += boost
        hk[:, j], hb[j] = hk[:, i], hb[i]
    return ws[:3] + [hk, hb.astype(np.float32)]


def underflow_weights(case):
    """the last class's bias raised until its logit leads every other by more than UNDERFLOW_LEAD on every clip of the restatement
    (the kernel of the head is untouched, so the other logits keep their spread): exp(-110) is 0 in float32, denormals included"""
    ws = weights(case)
    lg = reference(case)[0].astype(np.float64)
    hb = ws[4].copy()
    hb[-1] += np.float32(np.ceil((lg[:, :-1].max(1) - lg[:, -1]).max() + UNDERFLOW_LEAD + 10.0))
    return ws[:4] + [hb]
