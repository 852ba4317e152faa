"""Gradient parity that is exact about the model's DISCONTINUITIES.

simple_cnn's backward pass routes gradients through hard decisions -- ReLU6 gates (y in (0, 6)), the ReLU of conv4
(classifier/models/cnn.py:55), the max-pool arg-max.  A batch of useful size holds 10^5 .. 10^6 of them, and in the float64 oracle
the closest one sits within 1e-7 .. 1e-8 (relative) of its threshold in most batches: float32 device arithmetic may resolve
it the other way.  The forward value does not care, but ONE gradient element is then rerouted, and because the per-channel sums it
enters are sums of random-sign terms, a single rerouted element moves a bias-like gradient by up to ~1e-2 of its largest entry
(measured with tools/l1diag.py: B = 512, 2 of 3 batches, different elements in the fp32 and the split-bf16 paths).

So a device gradient is accepted when it matches the oracle's gradient for SOME resolution of the oracle's near-tie decisions: the
baseline, or the baseline with one (or two) of the decisions whose margin is below `eps` flipped -- re-running only the oracle's
backward pass with the flipped mask / arg-max entry.  Everything continuous still has to agree to the tight tolerance, and a
result that needs a flip reports which decision it was.
"""
import itertools

import numpy as np

from oracle import model_oracle as mo


def _rel_err(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


class TieAwareOracle(object):
    """One training forward + backward of `om` on (x, y) with the near-tie decisions recorded."""

    def __init__(self, om, x, y, class_weights=None, dropout_seed=None, eps=3e-6, max_candidates=6, ignore_index=None,
                 grad_scale=1.0, exact_ties=True):
        """exact_ties = False leaves out the ReLU6 / ReLU decisions whose margin is exactly 0 (tests/pool_tie_cases.py: both sides
        compute that value exactly there, so nothing is ambiguous about them)"""
        self.om = om
        rec, patched = {}, []
        for li, l in enumerate(om.layers):
            if isinstance(l, (mo.ReLU6, mo.MaxPool2)):
                f = l.forward

                def wrap(xx, training, _f=f, _li=li):
                    rec[_li] = xx
                    return _f(xx, training)
                l.forward = wrap                      # instance attribute shadows the method for this one pass
                patched.append(l)
        try:
            self.loss, self.acc, self.probs = mo.train_forward_backward(om, x, y, class_weights, dropout_seed, ignore_index=ignore_index,
                                                                           grad_scale=grad_scale)
        finally:
            for l in patched:
                del l.forward
        self.base = [g.copy() for g in om.grad_list()]
        self.inputs = rec                             # layer index -> input of every ReLU6 and MaxPool2 of the pass
        _, self.dlogits = mo.loss_and_grad(self.probs, y, class_weights, ignore_index, grad_scale)
        cands = []                                    # (relative margin, layer index, kind, index, payload)
        for li, l in enumerate(om.layers):
            if isinstance(l, mo.ReLU6):
                xin = rec[li]
                s = xin.std() + 1e-30
                for thr in (0.0, 6.0):
                    d = np.abs(xin - thr) / s
                    for i in np.argwhere(d < eps):
                        cands.append((float(d[tuple(i)]), li, "relu6", tuple(i), None))
            elif isinstance(l, mo.MaxPool2):
                xin = rec[li]
                B, H, W, C = xin.shape
                Ho, Wo = H // 2, W // 2
                win = np.stack([xin[:, 0:2 * Ho:2, 0:2 * Wo:2], xin[:, 0:2 * Ho:2, 1:2 * Wo:2], xin[:, 1:2 * Ho:2, 0:2 * Wo:2],
                                xin[:, 1:2 * Ho:2, 1:2 * Wo:2]], 0)
                order = np.argsort(-win, axis=0, kind="stable")
                top = np.take_along_axis(win, order[:2], 0)
                gap = (top[0] - top[1]) / (xin.std() + 1e-30)
                # gap > 0: an exact tie is no candidate for a flip.  Both sides see it, and "the first maximum wins" decides it:
                # tests/test_pool_ties_host.py and tests/test_pool_ties_gpu.py pin that rule, on data built to tie
                for i in np.argwhere((gap > 0) & (gap < eps)):
                    cands.append((float(gap[tuple(i)]), li, "pool", tuple(i), int(order[1][tuple(i)])))
            elif isinstance(l, mo.Conv2D) and l.relu:
                _, cols, _ = l.cache
                pre = cols @ l.kernel.reshape(-1, l.cout)
                d = np.abs(pre) / (pre.std() + 1e-30)
                for i in np.argwhere(d < eps):
                    cands.append((float(d[tuple(i)]), li, "relu", tuple(i), None))
        if not exact_ties:
            cands = [c for c in cands if c[0] > 0]
        cands.sort(key=lambda c: c[0])
        self.candidates = cands[:max_candidates]
        self.n_near_ties = len(cands)

    def _flip(self, cand):
        _, li, kind, idx, payload = cand
        l = self.om.layers[li]
        if kind == "relu6":
            l.mask[idx] = ~l.mask[idx]
            return lambda: l.mask.__setitem__(idx, ~l.mask[idx])
        if kind == "pool":
            old = int(l.arg[idx])
            l.arg[idx] = payload
            return lambda: l.arg.__setitem__(idx, old)
        y = l.cache[2]
        old = float(y[idx])
        y[idx] = 1e-300 if old == 0.0 else 0.0           # only the backward mask (y > 0) reads it now
        return lambda: y.__setitem__(idx, old)

    def alternatives(self):
        """(label, gradient list) for the baseline, every single flip, then pairs of the four closest decisions"""
        yield "baseline", self.base
        combos = [(c,) for c in self.candidates] + list(itertools.combinations(self.candidates[:4], 2))
        for combo in combos:
            undo = [self._flip(c) for c in combo]
            try:
                self.om.backward(self.dlogits)
                grads = [g.copy() for g in self.om.grad_list()]
            finally:
                for u in reversed(undo):
                    u()
            yield " + ".join("%s@layer%d%s (margin %.1e)" % (c[2], c[1], c[3], c[0]) for c in combo), grads
        self.om.backward(self.dlogits)                    # leave the oracle with its baseline gradients

    def match(self, device_grads, tol):
        """-> (matched, label of the matching alternative, worst relative error against it, error against the baseline)"""
        base_err = max(_rel_err(g, w) for g, w in zip(device_grads, self.base))
        best = (base_err, "baseline")
        if base_err >= tol:
            for label, grads in self.alternatives():
                err = max(_rel_err(g, w) for g, w in zip(device_grads, grads))
                if err < best[0]:
                    best = (err, label)
                if err < tol:
                    break
        return best[0] < tol, best[1], best[0], base_err
