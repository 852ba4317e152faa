"""Float64 numpy reference of the stacked simple_gru / simple_lstm (num_layers recurrent layers of 48 units -> Dense(C)), written
apart from the HIP kernels and from oracle.model_oracle's one-layer GRU / LSTM: layers that return their whole sequence, BPTT that takes
a gradient at every step and returns the input gradient, one input-dropout mask per layer.  Only the keep decision of the dropout hash
(oracle.model_oracle.dropout_keep), the softmax and the loss (softmax, loss_and_grad) are the oracle's.

Semantics (Keras, as the reference's classifier/models/rnn.py builds them): every layer is GRU(48, activation='linear', dropout=0.2) with
reset_after=True and bias (2, 144), gate order z, r, h -- or LSTM(48, activation='tanh', dropout=0.2), gate order i, f, c, o; every layer
but the last has return_sequences=True.  In training layer l multiplies its input by a mask of shape (B, F_l), shared by all steps:
keep / 0.8 with keep = dropout_keep(layer_seed(seed, l), B * F_l, 0.2) at index b * F_l + f.  seed == 0: no dropout in any layer.

No TensorFlow is installed where these tests run: parity with Keras itself is not pinned here, for the stacked models as for the
one-layer ones."""
import collections

import numpy as np

from oracle import model_oracle as mo

UNITS = 48
RATE = 0.2
GATES = {"simple_gru": 3, "simple_lstm": 4}
SEED_STEP = 0x9E3779B97F4A7C15      # include/kws.h: KWS_LAYER_DROPOUT_SEED(seed, l) = seed + l * SEED_STEP modulo 2^64


def layer_seed(seed, l):
    return (int(seed) + l * SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def layer_mask(seed, l, B, F, dtype=np.float64):
    """(B, F) mask of layer l: 0 or 1 / 0.8 (1.25, exact in float32 too); None when seed == 0"""
    if not seed:
        return None
    return (mo.dropout_keep(layer_seed(seed, l), B * F, RATE).reshape(B, F) / (1.0 - RATE)).astype(dtype)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


class SeqGRU(object):
    params = ("kernel", "recurrent_kernel", "bias")

    def __init__(self, cin, dtype):
        u = UNITS
        self.cin, self.dtype = cin, dtype
        self.kernel, self.recurrent_kernel, self.bias = np.zeros((cin, 3 * u), dtype), np.zeros((u, 3 * u), dtype), np.zeros((2, 3 * u), dtype)

    def forward(self, x, mask):
        """x (B, T, cin) -> every h_t (B, T, u)"""
        B, T, _ = x.shape
        u = UNITS
        xm = x if mask is None else x * mask[:, None, :]
        W, U, b = self.kernel, self.recurrent_kernel, self.bias
        h = np.zeros((B, u), self.dtype)
        seq = np.zeros((B, T, u), self.dtype)
        self.steps = []
        for t in range(T):
            mx, mh = xm[:, t] @ W + b[0], h @ U + b[1]
            z, r = _sig(mx[:, :u] + mh[:, :u]), _sig(mx[:, u:2 * u] + mh[:, u:2 * u])
            hh = mx[:, 2 * u:] + r * mh[:, 2 * u:]
            self.steps.append((h, z, r, hh, mh[:, 2 * u:]))
            h = z * h + (1 - z) * hh
            seq[:, t] = h
        self.xm, self.mask = xm, mask
        return seq

    def backward(self, dseq):
        """dseq (B, T, u): dL/dh_t arriving from above at every step -> dL/dx (B, T, cin); gradients in self.grads"""
        B, T, u = dseq.shape
        W, U = self.kernel, self.recurrent_kernel
        gW, gU, gb = np.zeros_like(W), np.zeros_like(U), np.zeros_like(self.bias)
        dx = np.zeros_like(self.xm)
        carry = np.zeros((B, u), self.dtype)
        for t in range(T - 1, -1, -1):
            h_prev, z, r, hh, mhh = self.steps[t]
            dh = carry + dseq[:, t]
            dhh = dh * (1 - z)
            dzp = dh * (h_prev - hh) * z * (1 - z)
            drp = dhh * mhh * r * (1 - r)
            dmx = np.concatenate([dzp, drp, dhh], 1)
            dmh = np.concatenate([dzp, drp, dhh * r], 1)
            gW += self.xm[:, t].T @ dmx
            gU += h_prev.T @ dmh
            gb[0] += dmx.sum(0)
            gb[1] += dmh.sum(0)
            dx[:, t] = dmx @ W.T
            carry = dh * z + dmh @ U.T
        self.grads = {"kernel": gW, "recurrent_kernel": gU, "bias": gb}
        return dx if self.mask is None else dx * self.mask[:, None, :]


class SeqLSTM(object):
    params = ("kernel", "recurrent_kernel", "bias")

    def __init__(self, cin, dtype):
        u = UNITS
        self.cin, self.dtype = cin, dtype
        self.kernel, self.recurrent_kernel, self.bias = np.zeros((cin, 4 * u), dtype), np.zeros((u, 4 * u), dtype), np.zeros((4 * u,), dtype)

    def forward(self, x, mask):
        B, T, _ = x.shape
        u = UNITS
        xm = x if mask is None else x * mask[:, None, :]
        h, c = np.zeros((B, u), self.dtype), np.zeros((B, u), self.dtype)
        seq = np.zeros((B, T, u), self.dtype)
        self.steps = []
        for t in range(T):
            a = xm[:, t] @ self.kernel + h @ self.recurrent_kernel + self.bias
            i, f, g, o = _sig(a[:, :u]), _sig(a[:, u:2 * u]), np.tanh(a[:, 2 * u:3 * u]), _sig(a[:, 3 * u:])
            cn = f * c + i * g
            tc = np.tanh(cn)
            self.steps.append((h, c, i, f, g, o, tc))
            h, c = o * tc, cn
            seq[:, t] = h
        self.xm, self.mask = xm, mask
        return seq

    def backward(self, dseq):
        B, T, u = dseq.shape
        W, U = self.kernel, self.recurrent_kernel
        gW, gU, gb = np.zeros_like(W), np.zeros_like(U), np.zeros_like(self.bias)
        dx = np.zeros_like(self.xm)
        carry, dc = np.zeros((B, u), self.dtype), np.zeros((B, u), self.dtype)
        for t in range(T - 1, -1, -1):
            h_prev, c_prev, i, f, g, o, tc = self.steps[t]
            dh = carry + dseq[:, t]
            dc = dc + dh * o * (1 - tc * tc)
            da = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            gW += self.xm[:, t].T @ da
            gU += h_prev.T @ da
            gb += da.sum(0)
            dx[:, t] = da @ W.T
            carry = da @ U.T
            dc = dc * f
        self.grads = {"kernel": gW, "recurrent_kernel": gU, "bias": gb}
        return dx if self.mask is None else dx * self.mask[:, None, :]


class StackedModel(object):
    def __init__(self, kind, num_classes, n_features, feature_size, num_layers, dtype=np.float64):
        if kind not in GATES:
            raise ValueError("Unsupported model type")
        self.kind, self.C, self.T, self.F, self.L, self.dtype = kind, num_classes, n_features, feature_size, num_layers, dtype
        cell = SeqGRU if kind == "simple_gru" else SeqLSTM
        self.rec = [cell(feature_size if l == 0 else UNITS, dtype) for l in range(num_layers)]
        self.head_kernel, self.head_bias = np.zeros((UNITS, num_classes), dtype), np.zeros((num_classes,), dtype)

    def width(self, l):
        return self.F if l == 0 else UNITS

    # ---- weights, Keras get_weights() order -------------------------------------------------------------------------
    def names(self):
        prefix = "gru_unit_" if self.kind == "simple_gru" else "lstm_unit_"
        return ["%s%d/%s" % (prefix, l, n) for l in range(self.L) for n in SeqGRU.params] + ["score_predict/kernel", "score_predict/bias"]

    def get_weights(self):
        return [np.array(getattr(r, n)) for r in self.rec for n in r.params] + [np.array(self.head_kernel), np.array(self.head_bias)]

    def set_weights(self, ws):
        assert len(ws) == 3 * self.L + 2
        it = iter(ws)
        for r in self.rec:
            for n in r.params:
                w = np.asarray(next(it), self.dtype)
                assert w.shape == getattr(r, n).shape, (n, w.shape)
                setattr(r, n, w.copy())
        self.head_kernel, self.head_bias = np.asarray(next(it), self.dtype).copy(), np.asarray(next(it), self.dtype).copy()

    def init_weights(self, seed=0, bias_noise=0.1):
        """Keras defaults (glorot-uniform kernels, per-gate orthogonal recurrent kernels, LSTM forget bias 1) with every bias moved off
        its initial value by bias_noise * N(0, 1)"""
        rng = np.random.default_rng(seed)
        ws = []
        for w, name in zip(self.get_weights(), self.names()):
            n = name.split("/")[1]
            if n == "kernel":
                lim = np.sqrt(6.0 / (w.shape[0] + w.shape[1]))
                v = rng.uniform(-lim, lim, w.shape)
            elif n == "recurrent_kernel":
                blocks = []
                for _ in range(w.shape[1] // UNITS):
                    q, r = np.linalg.qr(rng.standard_normal((UNITS, UNITS)))
                    blocks.append(q * np.sign(np.diag(r)))
                v = np.concatenate(blocks, 1)
            else:
                v = np.zeros(w.shape)
                if name.startswith("lstm"):
                    v[UNITS:2 * UNITS] = 1.0
                v = v + bias_noise * rng.standard_normal(w.shape)
            ws.append(v)
        self.set_weights(ws)
        return self

    # ---- compute ----------------------------------------------------------------------------------------------------
    def logits(self, x, seed=0, training=False):
        x = np.asarray(x, self.dtype)
        B = x.shape[0]
        for l, r in enumerate(self.rec):
            x = r.forward(x, layer_mask(seed, l, B, self.width(l), self.dtype) if training else None)
        self.h_last = x[:, -1]
        return self.h_last @ self.head_kernel + self.head_bias

    def predict(self, x):
        return mo.softmax(self.logits(x))

    def losses(self, x, labels, class_weights=None, seed=0):
        """per-sample losses, probabilities and dlogits of a training pass"""
        p = mo.softmax(self.logits(x, seed, training=True))
        cw = None if class_weights is None else np.asarray(class_weights, self.dtype)
        losses, dlogits = mo.loss_and_grad(p, labels, cw)
        return losses, p, dlogits

    def train_forward_backward(self, x, labels, class_weights=None, seed=0):
        """-> (mean loss, correct predictions, probabilities); gradients in grad_list(), input gradient in self.dx"""
        losses, p, dlogits = self.losses(x, labels, class_weights, seed)
        self.g_head = (self.h_last.T @ dlogits, dlogits.sum(0))
        d = np.zeros((x.shape[0], self.T, UNITS), self.dtype)
        d[:, -1] = dlogits @ self.head_kernel.T
        for r in reversed(self.rec):
            d = r.backward(d)
        self.dx = d
        return float(losses.mean()), int((p.argmax(-1) == np.asarray(labels).reshape(-1)).sum()), p

    def grad_list(self):
        return [r.grads[n] for r in self.rec for n in r.params] + list(self.g_head)


Result = collections.namedtuple("Result", "weights infer_probs loss correct probs grads names losses")


def run(model, x, labels, class_weights, seed):
    """inference and one training pass -> Result (rnn_cases.compare reads it: names[0] / grads[0] are layer 0's input kernel)"""
    x = np.asarray(x, model.dtype)
    with np.errstate(over="ignore"):
        infer = model.predict(x)
        losses = model.losses(x, labels, class_weights, seed)[0]
        loss, correct, probs = model.train_forward_backward(x, labels, class_weights, seed)
    return Result(model.get_weights(), infer, loss, correct, probs, [np.array(g) for g in model.grad_list()], model.names(), losses)
