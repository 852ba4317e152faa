"""float64 numpy oracle of the tf.keras optimizer_v2 updates kws_optimizer_step implements (include/kws.h): gradient clipping by
value, per-variable norm (tf.clip_by_norm) and global norm (tf.clip_by_global_norm), SGD momentum / nesterov, RMSprop momentum /
centered, Adam amsgrad."""
import numpy as np


def clip_by_norm(g, c):
    """tf.clip_by_norm: g*c / max(||g||, c); a zero norm leaves g, an inf norm makes finite entries 0 and inf entries NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        l2sum = np.sum(g * g)
        norm = np.sqrt(l2sum) if l2sum > 0 else l2sum
        return g * c / np.maximum(norm, c)


def clip_by_global_norm(gs, c):
    """tf.clip_by_global_norm over a list of arrays; a non-finite global norm makes every entry NaN"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = np.sqrt(sum(np.sum(g * g) for g in gs))
        scale = c * min(1.0 / n, 1.0 / c) if np.isfinite(n) else np.nan
        return [g * scale for g in gs]


class RefOptimizer(object):
    """kind in {'sgd', 'rmsprop', 'adam'}; `beta2` is RMSprop's rho.  step(p, g, segments) updates p (float64) in place."""

    def __init__(self, kind, lr, beta1=0.9, beta2=0.999, eps=1e-7, momentum=0.0, nesterov=False, centered=False, amsgrad=False,
                 clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0):
        self.kind, self.lr, self.beta1, self.beta2, self.eps = kind, lr, beta1, beta2, eps
        self.momentum, self.nesterov, self.centered, self.amsgrad = momentum, nesterov, centered, amsgrad
        self.clipvalue, self.clipnorm, self.global_clipnorm = clipvalue, clipnorm, global_clipnorm
        self.t = 0
        self.slots = {}

    def slot(self, name, like):
        if name not in self.slots:
            self.slots[name] = np.zeros_like(like, dtype=np.float64)
        return self.slots[name]

    def transform(self, g, segments):
        g = np.asarray(g, np.float64).copy()
        if self.clipvalue:
            g = np.clip(g, -self.clipvalue, self.clipvalue)
        if self.clipnorm:
            for o, n in segments:
                g[o:o + n] = clip_by_norm(g[o:o + n], self.clipnorm)
        if self.global_clipnorm:
            parts = clip_by_global_norm([g[o:o + n] for o, n in segments], self.global_clipnorm)
            for (o, n), q in zip(segments, parts):
                g[o:o + n] = q
        return g

    def step(self, p, g, segments):
        self.t += 1
        g = self.transform(g, segments)
        lr, mu = self.lr, self.momentum
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.kind == "sgd":
                if mu > 0:
                    a = self.slot("mom", p)
                    a[:] = mu * a - lr * g
                    p += mu * a - lr * g if self.nesterov else a
                else:
                    p -= lr * g
            elif self.kind == "rmsprop":
                rho = self.beta2
                ms = self.slot("v", p)
                ms[:] = rho * ms + (1 - rho) * g * g
                d = ms
                if self.centered:
                    mg = self.slot("mg", p)
                    mg[:] = rho * mg + (1 - rho) * g
                    d = ms - mg * mg
                if mu > 0:
                    mom = self.slot("mom", p)
                    mom[:] = mu * mom + lr * g / np.sqrt(d + self.eps)
                    p -= mom
                else:
                    p -= lr * g / (np.sqrt(d) + self.eps)
            else:
                b1, b2, t = self.beta1, self.beta2, self.t
                m, v = self.slot("m", p), self.slot("v", p)
                m[:] = b1 * m + (1 - b1) * g
                v[:] = b2 * v + (1 - b2) * g * g
                lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
                if self.amsgrad:
                    vh = self.slot("vhat", p)
                    vh[:] = np.maximum(vh, v)
                    p -= lr_t * m / (np.sqrt(vh) + self.eps)
                else:
                    p -= lr_t * m / (np.sqrt(v) + self.eps)
        return p
