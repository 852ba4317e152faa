"""Helpers of tests/test_loss_options_gpu.py: the train step's head sites (which kernel computes loss and dlogits, from the dispatch of
kws_model.hip / kws_rnn.hip), one model per site row with its oracle and device steps, label builders (a class with a given share of
the batch; one label per clip in a chosen zone of the plain loss's clip gate) and the comparison with the float64 oracle at the
tolerances of tests/test_heads_gpu.py."""
import numpy as np

from head_cases import device_model, features, float_model, head_forms, head_inputs
from oracle import model_oracle as mo

RNN = ("simple_gru", "simple_lstm")

# (site, kind, C, mode): mode None = defaults, "fp32" = set_precision(matrix=MATRIX_FP32), "det" = set_deterministic(True)
ROWS = [("fused", "simple_cnn", 5, None), ("fused", "simple_cnn", 48, None),
        ("mfma", "simple_gru", 12, None), ("mfma", "simple_lstm", 48, None), ("mfma", "simple_cnn", 17, "fp32"),
        ("fast", "simple_cnn", 49, None), ("fast", "simple_cnn_lite", 12, None), ("fast", "simple_gru", 100, None),
        ("fast", "simple_cnn", 17, "det"),
        ("slow", "simple_cnn", 100, None), ("slow", "simple_lstm", 300, None), ("slow", "simple_gru", 1024, None)]
ROW_IDS = ["%s-%s-%d%s" % (s, k, C, "-" + m if m else "") for s, k, C, m in ROWS]


def train_head_site(kind, K, C, matrix_bf16=True, deterministic=False):
    """the kernel that computes loss and dlogits in a train step (kws_model_train_fwd_bwd, gru_train_fwd_bwd):
    "fused" dense_head_fused_kernel, "mfma" head_bwd_mfma_kernel<.., FWD>, "fast" head_fwd_fast_kernel, "slow" head_fwd_kernel"""
    f = head_forms(kind, K, C, matrix_bf16)
    if kind == "simple_cnn" and f["mfma_bwd"] and not deterministic:
        return "fused" if f["fused_tail"] else "mfma"          # CnnPlan::dense_fused: split-bf16 matrix mode, else the FWD head
    if kind in RNN and f["mfma_bwd"]:
        return "mfma"
    return "fast" if f["fast_fwd"] else "slow"


class Step(object):
    """what one device step left: stats (numpy), probabilities (numpy), the gradient and state buffers (device clones)"""

    def __init__(self, stats, probs, grads, state, grad_list, weights):
        self.stats, self.probs, self.grads, self.state, self.grad_list, self.weights = stats, probs, grads, state, grad_list, weights


class Ref(object):
    """the oracle's step: mean loss, accuracy, probabilities, gradients (tie-aware for simple_cnn), weights after the step"""


class Case(object):
    def __init__(self, torch, site, kind, C, mode, spread=1.5, seed=None):
        from kws_amd import lib as L
        self.torch, self.site, self.kind, self.C, self.mode = torch, site, kind, C, mode
        self.om = float_model(kind, C, seed=C if seed is None else seed, spread=spread)
        self.w0 = [np.array(w) for w in self.om.get_weights()]
        self.dm = device_model(self.om)
        self.det = mode == "det"
        if mode == "fp32":
            self.dm.set_precision(matrix=L.MATRIX_FP32)
            assert self.dm.get_precision()[0] == L.MATRIX_FP32
        elif kind == "simple_cnn":
            assert self.dm.get_precision()[0] == L.MATRIX_BF16X6
        if self.det:
            self.dm.set_deterministic(True)
        K = self.dm.spec.tensors[-2]["shape"][0]
        assert self.dm.spec.tensors[-2]["name"] == "score_predict/kernel" and K == head_inputs(kind)
        assert train_head_site(kind, K, C, mode != "fp32", self.det) == site, (site, kind, C, mode)
        if site == "slow" and C == 1024:
            assert head_forms(kind, K, C)["slow_lds"] > 64 * 1024
        self.state0 = self.dm.state.clone()
        self.has_state = self.dm.spec.state_count > 0

    def set_head_bias(self, bias):
        self.w0[-1] = np.asarray(bias, np.float32)
        self.om.set_weights(self.w0)
        self.dm.set_weights(self.w0)
        self.state0 = self.dm.state.clone()

    def train_logits(self, x, seed):
        """the oracle's training-mode logits (they do not depend on the labels), float64"""
        self.om.set_weights(self.w0)
        self.om.set_dropout(seed if seed else None, None)
        z = self.om.logits(x.astype(np.float64), training=True)
        self.om.set_weights(self.w0)
        return z

    def let_class_win(self, k, x, seed, clips=4):
        """raise class k's bias so that it is the arg-max of at least `clips` clips of the training forward pass: clips labelled k
        (masked under ignore_index = k) are then among the hits"""
        z = self.train_logits(x, seed)
        other = np.delete(z, k, axis=1).max(-1)
        bias = self.w0[-1].astype(np.float64)
        bias[k] += max(0.0, np.sort(other - z[:, k])[clips - 1] + 0.01)
        self.set_head_bias(bias)

    def oracle(self, x, y, cw, seed, ignore_index=None, grad_scale=1.0):
        self.om.set_weights(self.w0)                       # the moving statistics of the step before are gone
        r = Ref()
        x64 = x.astype(np.float64)
        if self.kind == "simple_cnn":
            from tie_aware import TieAwareOracle
            r.tao = TieAwareOracle(self.om, x64, y, cw, seed if seed else None, ignore_index=ignore_index, grad_scale=grad_scale)
            r.loss, r.acc, r.probs, r.grads = r.tao.loss, r.tao.acc, r.tao.probs, r.tao.base
        else:
            r.tao = None
            r.loss, r.acc, r.probs = mo.train_forward_backward(self.om, x64, y, cw, dropout_seed=seed if seed else None,
                                                               ignore_index=ignore_index, grad_scale=grad_scale)
            r.grads = [g.copy() for g in self.om.grad_list()]
        r.weights = [np.array(w) for w in self.om.get_weights()]
        return r

    def device(self, x, y, cw, seed, **kw):
        torch, dm = self.torch, self.dm
        dm.state.copy_(self.state0)
        cwd = torch.from_numpy(np.asarray(cw, np.float32)).cuda() if cw is not None else None
        probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(np.asarray(y).astype(np.int32)).cuda(), cwd, dropout_seed=seed,
                                 want_probs=True, **kw)
        torch.cuda.synchronize()
        return Step(dm.stats.cpu().numpy().copy(), probs.cpu().numpy(), dm.grads.clone(), dm.state.clone(), dm.get_grads(), dm.get_weights())

    def check(self, step, ref, what, loss_tol=1e-4):
        """the tolerances of tests/test_heads_gpu.py: probabilities 1e-4 absolute, mean loss 1e-4, hits exact, every gradient tensor 3e-4 of
        its largest entry (tie-aware for simple_cnn; the lite pointwise-bias floor 1e-6).  Prints each figure before it asserts."""
        B = len(ref.probs)
        perr = float(np.abs(step.probs - ref.probs).max())
        lerr = abs(float(step.stats[0]) / B - ref.loss)
        if self.kind == "simple_cnn":
            ok, label, gerr, base_err = ref.tao.match(step.grad_list, 3e-4)
            worst = (gerr, label)
        else:
            ok, worst = True, (0.0, "")
            names = [w for w in self.om.weight_list() if w[2]]
            for t, (g, want, (li, n, _)) in enumerate(zip(step.grad_list, ref.grads, names)):
                scale, floor = float(np.abs(want).max()), (1e-6 if self.kind == "simple_cnn_lite" else 0.0)
                if n == "bias" and isinstance(self.om.layers[li], mo.SeparableConv2D):
                    scale = float(np.abs(ref.grads[t - 1]).max())          # an exactly-zero gradient: measured against its layer's kernel
                err = float(np.abs(g - want).max())
                rel = max(err - floor, 0.0) / (scale + 1e-300)
                if rel > worst[0]:
                    worst = (rel, "layer %d %s" % (li, n))
                ok = ok and err < 3e-4 * scale + floor
        print("FIGURES %s %s C=%d %s | %s: probs %.3g (1e-4)  loss %.3g (%.3g)  hits %d/%d  grads %.3g (3e-4) %s"
              % (self.site, self.kind, self.C, self.mode or "default", what, perr, lerr, loss_tol, int(step.stats[1]), round(ref.acc * B),
                 worst[0], worst[1]))
        assert perr < 1e-4, (what, perr)
        assert lerr < loss_tol, (what, float(step.stats[0]) / B, ref.loss)
        assert step.stats[1] == round(ref.acc * B), (what, step.stats[1], ref.acc * B)
        assert ok, (what, "gradients", worst)

    def check_state(self, step, ref, moved=True):
        """BatchNormalization moving statistics as the oracle's after the step (tests/test_model_gpu.py's bound), and not where they were"""
        for i, (li, n, t) in enumerate(self.om.weight_list()):
            if not t:
                np.testing.assert_allclose(step.weights[i], ref.weights[i], rtol=2e-5, atol=1e-6, err_msg=n)
                if moved:
                    assert not np.allclose(step.weights[i], self.w0[i], rtol=1e-6, atol=1e-7), n

    def same_grads(self, a, b, what, exact):
        """bit-equal gradient buffers, or (float atomics, tests/test_model_gpu.py) within 2e-5 of the largest entry"""
        torch = self.torch
        if exact:
            assert torch.equal(a, b), (what, float((a - b).abs().max()))
        else:
            scale = float(b.abs().max())
            err = float((a - b).abs().max())
            print("FIGURES %s %s C=%d | %s: gradient order noise %.3g of the largest entry (2e-5)" % (self.site, self.kind, self.C, what,
                                                                                                     err / (scale + 1e-300)))
            assert err <= 2e-5 * scale, (what, err, scale)


# ---- labels -------------------------------------------------------------------------------------------------------------
def labels_with_share(rng, B, C, k, first=(), share=0.3):
    """random labels in which class k holds `share` of the batch (the clips `first` among them) and 0 and C - 1 are both present"""
    y = rng.integers(0, C, B)
    y[y == k] = (k + 1) % C
    n = int(round(share * B))
    order = list(first) + [i for i in rng.permutation(B) if i not in set(first)]
    y[order[:n]] = k
    y[order[n]], y[order[n + 1]] = 0, C - 1
    assert 0.2 * B <= (y == k).sum() <= 0.4 * B and (y == 0).any() and (y == C - 1).any() and k > 0
    return y


OPEN, WRONG, RIGHT = 0, 1, 2


def gate_zones(p):
    """per clip, from float64 probabilities: the labels that put it in the open zone (1e-5 < p_y < 1 - 1e-5), in the confidently-wrong
    zone (1e-30 < p_y < 1e-8), and whether its arg-max is confidently right (the other classes sum to less than 2e-8)"""
    out = []
    for row in p:
        am = int(row.argmax())
        rest = float(np.delete(row, am).sum())
        out.append((np.nonzero((row > 1e-5) & (row < 1 - 1e-5))[0], np.nonzero((row > 1e-30) & (row < 1e-8))[0], am if rest < 2e-8 else None))
    return out


def gate_labels(p, rng):
    """one label per clip so that every clip lies in a zone: the confidently-right clips first, then the zone that is shortest so far
    among those the clip can reach.  -> (labels, zone of every clip); None if a clip reaches no zone"""
    B = len(p)
    y, zone = np.zeros(B, np.int64), np.zeros(B, np.int64)
    count = [0, 0, 0]
    zs = gate_zones(p)
    for b in sorted(range(B), key=lambda i: zs[i][2] is None):
        op, wr, rt = zs[b]
        if rt is not None and count[RIGHT] <= min(count[OPEN], count[WRONG]) + 2:
            y[b], zone[b] = rt, RIGHT
        elif len(op) and (count[OPEN] <= count[WRONG] or not len(wr)):
            y[b], zone[b] = rng.choice(op), OPEN
        elif len(wr):
            y[b], zone[b] = rng.choice(wr), WRONG
        elif rt is not None:
            y[b], zone[b] = rt, RIGHT
        else:
            return None
        count[zone[b]] += 1
    return y, zone


def assert_zones(p, y, zone):
    """on the oracle: every clip in exactly the zone it was labelled for, none in the bands between, at least 3 per zone"""
    py = p[np.arange(len(y)), y]
    rest = p.sum(-1) - py
    in_open = (py > 1e-5) & (py < 1 - 1e-5)
    in_wrong = (py > 1e-30) & (py < 1e-8)
    in_right = np.array([np.delete(p[b], y[b]).sum() < 2e-8 for b in range(len(y))])
    assert np.all(in_open == (zone == OPEN)) and np.all(in_wrong == (zone == WRONG)) and np.all(in_right == (zone == RIGHT)), (py, rest, zone)
    assert np.all(in_open.astype(int) + in_wrong + in_right == 1)
    assert min((zone == z).sum() for z in (OPEN, WRONG, RIGHT)) >= 3, [(zone == z).sum() for z in (OPEN, WRONG, RIGHT)]
