"""Case table of the stacked recurrent models (tests/test_rnn_stack_gpu.py, tests/test_rnn_stack_host.py): simple_gru / simple_lstm with
num_layers = 2 .. 4 (kws_model_create_stacked), against tests/rnn_stack_ref.py.

Layer 0 runs the kernel templates of the one-layer models with SEQ / DSEQ set, every layer above runs the KX = 12 instantiations on the
48-wide sequence of the layer below (csrc/kws_rnn.hip: dispatch_fwd, dispatch_bwd).  The launch arithmetic is tests/rnn_cases.py's,
applied per layer: layer l stages a 16-clip tile of T x F_l floats (F_0 = F, F_l = 48 above), and every layer's tiles are checked before
anything is launched.  With F_l = 48:

    T    XS = T * 48 -> 18 mod 32    forward 4 (16 XS + 4800) B    backward 4 (16 XS + 5760) B
    9    434                          46 976                        50 816        neither launch opts in (<= 65 536)
    14   690                          63 360                        67 200        only the backward launch opts in
    30   1458                         112 512                       116 352       both opt in
    45   2162                         157 568                       161 408       the longest sequence that trains (<= 163 840)
    46   2226                         161 664                       165 504       inference runs, the train step is refused

Everything here is host-only."""
import collections

import numpy as np

import rnn_cases as rc
import rnn_stack_ref as sr

KINDS = rc.KINDS
UPPER_F = sr.UNITS               # input width of layers 1 .. num_layers - 1
UPPER_KX = 12                    # their template
LONGEST_TRAIN_T = 45
REFUSED_TRAIN_T = 46

Case = collections.namedtuple("Case", "label kind L T F B C class_weights dropout_seed")


def layer_width(case, l):
    return case.F if l == 0 else UPPER_F


def layer_branch(case, l):
    """(KX, forward opts in, backward opts in) of layer l"""
    F = layer_width(case, l)
    return (rc.kx_for(F) if l == 0 else UPPER_KX), rc.fwd_opts_in(case.T, F), rc.bwd_opts_in(case.T, F)


def branch(case):
    """(layer 0's branch, the upper layers' branch, head fused)"""
    return layer_branch(case, 0), layer_branch(case, 1), rc.head_bwd_fuses(case.C)


def infer_supported(case):
    return all(rc.infer_supported(case.T, layer_width(case, l)) for l in range(case.L))


def train_supported(case):
    return all(rc.train_supported(case.T, layer_width(case, l)) for l in range(case.L))


# every combination the table is there to run, for each kind
REQUIRED_BRANCHES = {
    ((5, False, False), (12, False, False), True),       # T = 9: no launch opts in
    ((10, False, False), (12, False, False), True),      # F = 37
    ((16, False, False), (12, False, False), True),      # F = 64
    ((5, False, False), (12, False, True), True),        # T = 14: only the upper layers' backward launch
    ((5, False, False), (12, True, True), True),         # T = 39 x 13: the upper layers opt in, layer 0 does not
    ((5, True, True), (12, True, True), True),           # T = 45 x 20: both of layer 0's launches too
    ((5, False, False), (12, False, False), False),      # C = 49: head forward, memset, head backward
}


def _cases():
    cases = []
    for kind in KINDS:
        k = kind[len("simple_"):]

        def add(label, L, T, F, B, C=6, cw=None, seed=None):
            cases.append(Case("%s%d-%s" % (k, L, label), kind, L, T, F, B, C, cw, 4242 + T + L if seed is None else seed))
        for L in (2, 3):
            # sequence edges: at T = 1 every dU is exactly zero and the lower layers' only gradient arrives through dseq
            for T in (1, 2):
                add("steps%d" % T, L, T, 20, 17)
            # batch edges around the 16-clip tile
            for B in (1, 15, 17, 33):
                add("batch%d" % B, L, 9, 20, B)
            # layer-0 widths on both sides of 48, and one in the KX = 10 template
            for F in (3, 37, 64):
                add("width%d" % F, L, 9, F, 17)
            # both head chains, class weights, dropout seeds
            add("classes49", L, 9, 20, 17, C=49)
            add("weighted", L, 9, 20, 17, cw=rc._weights(6))
            add("seed0", L, 9, 20, 17, seed=0)
            add("seed_wide", L, 9, 20, 17, seed=rc.WIDE_SEED)
            # LDS edges of the 48-wide layers: backward launch alone above 64 KiB; the longest sequence that trains
            add("lds14", L, 14, 20, 17)
            add("lds%d" % LONGEST_TRAIN_T, L, LONGEST_TRAIN_T, 20, 17)
        add("demo39x13", 2, 39, 13, 17)                  # the shape of the reference's own rnn.py demo
        add("four", 4, 5, 20, 17)
    return cases


CASES = _cases()
CASE = {c.label: c for c in CASES}


def refused_train_case(kind, L=2):
    return Case("%s%d-refused" % (kind[len("simple_"):], L), kind, L, REFUSED_TRAIN_T, 20, 17, 6, None, 4242 + REFUSED_TRAIN_T)


def shrink_cases(kind, L=2):
    k = kind[len("simple_"):]
    return (Case("%s%d-shrink-first" % (k, L), kind, L, 9, 20, rc.SHRINK[0], 6, None, 4251),
            Case("%s%d-shrink" % (k, L), kind, L, 9, 20, rc.SHRINK[1], 6, None, 4250))


def one_layer_case(kind):
    return Case("%s1-identity" % kind[len("simple_"):], kind, 1, 9, 20, 17, 6, None, 4251)


# ---- tolerances -------------------------------------------------------------------------------------------------------
# rnn_cases' own (PROB_ATOL, LOSS_ATOL, GRAD_RTOL and its row bound) for every tensor of every case: the float32 run of the reference
# stays within a tenth of each of them on the whole table (tests/test_rnn_stack_host.py: test_float32_reference_... asserts it and
# prints the figures; the largest on this table are recorded there).  No tensor needed a bound of its own.
FLOAT32_MARGIN = 10
LABEL_PROB_FLOOR = 1e-5
HEAD_GAIN = {"simple_gru": 1.0, "simple_lstm": 4.0}      # the GRU's linear activation needs none: its states grow with depth


# ---- builders ---------------------------------------------------------------------------------------------------------
def model(case, dtype=np.float64):
    """Keras-default initialisation of the recurrent layers with the biases moved off their initial values, rounded to the float32 values
    the device holds; the LSTM cases' head is NOT the Keras default.  The LSTM head's kernel is HEAD_GAIN times its glorot draw: the last state of a deep stack is small (an LSTM's |h| < 1 shrinks from layer
    to layer), and with 49 classes the glorot head leaves every probability within a few 1e-4 of 1 / 49 -- no feature seed then separates
    the two best classes of all 17 clips by the margin reference() asks for."""
    init = sr.StackedModel(case.kind, case.C, case.T, case.F, case.L).init_weights(1000 * case.L + case.T + case.F)
    ws = init.get_weights()
    ws[-2] = ws[-2] * HEAD_GAIN[case.kind]
    out = sr.StackedModel(case.kind, case.C, case.T, case.F, case.L, dtype)
    out.set_weights([w.astype(np.float32) for w in ws])
    return out


def _inputs(case, salt):
    rng = np.random.default_rng(case.T * 100 + case.F + 7 * case.B + 1000 * case.L + 100000 * salt)
    x = rng.standard_normal((case.B, case.T, case.F)) * 2.0
    x[..., 0] -= 10.0                                   # an MFCC-like c0 column
    y = rng.integers(0, case.C, case.B)
    cw = None if case.class_weights is None else np.array(case.class_weights)
    return x.astype(np.float32), y, cw


_REFERENCES = {}


def _margin(p):
    s = np.sort(p, -1)
    return float((s[:, -1] - s[:, -2]).min())


def reference(case):
    """(inputs, float64 Result), computed once per case.  The feature seed is moved on the float64 reference alone: a case takes the first
    salt at which every clip's two best classes are more than twice the probability tolerance apart, at inference and in the training
    pass -- an arg-max or a correct count cannot then turn on float32 rounding -- and every clip's label keeps a probability above
    LABEL_PROB_FLOOR, a hundred times the 1e-7 at which the loss clips and passes no gradient (a stacked linear-activation GRU saturates
    its softmax easily; a clipped clip would test nothing).  No device output is involved."""
    if case not in _REFERENCES:
        m = model(case)
        for salt in range(256):
            x, y, cw = _inputs(case, salt)
            res = sr.run(m, x, y, cw, case.dropout_seed)
            if min(_margin(res.infer_probs), _margin(res.probs)) > 2 * rc.PROB_ATOL and res.probs[np.arange(case.B), y].min() > LABEL_PROB_FLOOR:
                break
        else:
            raise AssertionError("no feature seed leaves %s clear of ties" % case.label)
        _REFERENCES[case] = ((x, y, cw), res)
    return _REFERENCES[case]


def run_float32(case):
    (x, y, cw), _ = reference(case)
    return sr.run(model(case, np.float32), x, y, cw, case.dropout_seed)
