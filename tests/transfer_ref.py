"""Numpy restatement of kws_head_fit / kws_amd.transfer.fit_head (include/kws.h): a Dense(E -> C, softmax) head trained on fixed
embeddings, built from oracle/model_oracle.py's softmax, loss_and_grad and Adam plus an SGD-momentum rule.  float64 by default; `dtype`
runs the same statements in float32, and `reverse` sums every batch in the opposite row order -- the two float32 runs the GPU tests
derive their tolerance from and check their seeds with (tests/transfer_cases.py)."""
import numpy as np

from oracle import model_oracle as mo


class SgdMomentum(object):
    """keras.optimizers.SGD(lr, momentum, nesterov=False): momentum 0: w -= lr g; else v = momentum v - lr g, w += v"""

    def __init__(self, lr, momentum=0.0):
        self.lr, self.momentum, self.v = lr, momentum, None

    def step(self, params, grads, lr=None):
        lr = self.lr if lr is None else lr
        if self.v is None:
            self.v = [np.zeros_like(p) for p in params]
        out = []
        for i, (p, g) in enumerate(zip(params, grads)):
            dt = p.dtype.type
            if self.momentum > 0:
                self.v[i] = dt(self.momentum) * self.v[i] - dt(lr) * g
                out.append(p + self.v[i])
            else:
                out.append(p - dt(lr) * g)
        return out


class HeadState(object):
    """what a launch carries to the next: weights, optimizer slots, Adam's step count"""

    def __init__(self, kernel, bias, dtype=np.float64):
        self.kernel, self.bias = np.asarray(kernel, dtype).copy(), np.asarray(bias, dtype).copy()
        self.m = [np.zeros_like(self.kernel), np.zeros_like(self.bias)]
        self.v = [np.zeros_like(self.kernel), np.zeros_like(self.bias)]
        self.t = 0
        self.dtype = dtype

    def copy(self, dtype=None):
        out = HeadState(self.kernel, self.bias, dtype or self.dtype)
        out.m = [np.asarray(a, out.dtype).copy() for a in self.m]
        out.v = [np.asarray(a, out.dtype).copy() for a in self.v]
        out.t = self.t
        return out


def fit_launch(emb, labels, order, batch, state, optimizer="adam", lr=1e-3, momentum=0.0, class_weights=None, ignore_index=0,
               beta1=0.9, beta2=0.999, eps=1e-7, reverse=False):
    """One kws_head_fit job: walks `order` in steps of `batch` (the last step takes the rest, its mean runs over its own size) and
    updates `state` in place.  -> (sum of the per-sample losses, number of top-1 hits) over all steps.  An empty order changes nothing."""
    dt = state.dtype
    emb = np.asarray(emb, dt)
    labels = np.asarray(labels).reshape(-1)
    order = np.asarray(order, np.int64)
    cw = None if class_weights is None else np.asarray(class_weights, dt)
    loss_sum, hits = dt(0), 0.0
    for s in range(0, len(order), batch):
        rows = order[s:s + batch]
        if reverse:
            rows = rows[::-1]
        x, y = emb[rows], labels[rows]
        p = mo.softmax(x @ state.kernel + state.bias)
        losses, dlogits = mo.loss_and_grad(p, np.where(y < p.shape[1], y, 0), cw, None)
        if ignore_index and ignore_index > 0:
            # applied here, not in loss_and_grad, so that an ignored label may lie outside [0, C)
            masked = y == ignore_index
            losses = np.where(masked, dt(0), losses)
            dlogits = np.where(masked[:, None], dt(0), dlogits)
        grads = [x.T @ dlogits, dlogits.sum(0)]
        loss_sum = dt(loss_sum + losses.sum(dtype=dt))          # stats are `dtype` values: a float32 run carries a float32 sum
        hits += float((p.argmax(-1) == y).sum())
        if optimizer == "adam":
            opt = mo.Adam(lr, beta1, beta2, eps)
            opt.m, opt.v, opt.t = state.m, state.v, state.t
            new = opt.step([state.kernel, state.bias], grads)
            if dt != np.float64:
                # the kernel's update in float32: the bias correction is a double expression cast to float (kws_adam_step)
                t = state.t + 1
                lr_t = dt(lr * np.sqrt(1 - float(dt(beta2)) ** t) / (1 - float(dt(beta1)) ** t))
                new = [p_ - lr_t * m_ / (np.sqrt(v_) + dt(eps)) for p_, m_, v_ in zip([state.kernel, state.bias], opt.m, opt.v)]
            state.m, state.v, state.t = [np.asarray(a, dt) for a in opt.m], [np.asarray(a, dt) for a in opt.v], opt.t
        elif optimizer == "sgd":
            opt = SgdMomentum(lr, momentum)
            opt.v = state.m
            new = opt.step([state.kernel, state.bias], grads)
            state.m = opt.v
            state.t += 1
        else:
            raise ValueError("optimizer %r" % (optimizer,))
        state.kernel, state.bias = np.asarray(new[0], dt), np.asarray(new[1], dt)
    return float(loss_sum), hits


def fit_head(emb, labels, num_classes, orders, batch, kernel, bias, lrs, dtype=np.float64, **kw):
    """fit_head of kws_amd.transfer driven with explicit per-epoch orders and learning rates -> (HeadState, [mean loss], [accuracy])"""
    st = HeadState(kernel, bias, dtype)
    loss, acc = [], []
    for order, lr in zip(orders, lrs):
        s, h = fit_launch(emb, labels, order, batch, st, lr=lr, **kw)
        loss.append(s / len(order))
        acc.append(h / len(order))
    return st, loss, acc
