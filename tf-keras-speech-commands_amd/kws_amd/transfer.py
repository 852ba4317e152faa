"""Transfer to a new keyword set on a frozen backbone (include/kws.h: kws_model_embed, kws_head_fit).

    emb = embed(model, x)                          # (N, E) activations in front of score_predict, computed once
    head = fit_head(emb, y, num_classes, epochs=10, lr=1e-3)
    new_model = with_head(model, head)             # a KWSModel of the new class count: predict / evaluate / quantize / save / streams

`fit_heads` trains many independent heads in ONE launch (one block each), `cross_validate` is built on it.  `HeadBank` keeps many
fitted heads on the device and applies to every row the head that row names (kws_heads_apply): `score_heads` scores every head on its
own rows in one launch, and kws_amd.stream serves a keyword set per stream from a bank.  torch is device memory and
the stream only; the head's arithmetic is the kernel's.  Everything is validated on the host before any device work (ValueError): the
kernel trusts the `order` and `labels` it is given."""
import ctypes

import numpy as np

from . import lib as _l

ADAM_DEFAULTS = dict(beta1=0.9, beta2=0.999, eps=1e-7)      # keras.optimizers.Adam


def max_classes(E):
    """kws_head_fit_max_classes: the most classes a head on E-wide embeddings may have (0: E itself is not supported)"""
    return int(_l.get_lib().kws_head_fit_max_classes(int(E)))


def glorot_head(E, C, seed=None):
    """Keras' Dense defaults: glorot_uniform kernel (E, C), zero bias"""
    lim = np.sqrt(6.0 / (E + C))
    return np.random.default_rng(seed).uniform(-lim, lim, (E, C)).astype(np.float32), np.zeros((C,), np.float32)


class HeadFit(object):
    """A trained head.  kernel (E, C) / bias (C): numpy float32 in Keras Dense layout; loss / accuracy: one value per epoch (the mean of
    the per-sample losses / the share of top-1 hits over the epoch's rows); state: what a later fit_head(init=head, state=head.state)
    continues from -- the optimizer, its step count t and its slots m / v as flat device tensors in the layout of the weights."""

    def __init__(self, num_classes, embed_size, weights, state, loss, accuracy):
        self.num_classes, self.embed_size = int(num_classes), int(embed_size)
        self.weights = weights                  # flat device tensor: kernel (E, C) row-major, then bias (C)
        self.state = state
        self.loss, self.accuracy = list(loss), list(accuracy)

    @property
    def kernel(self):
        E, C = self.embed_size, self.num_classes
        return self.weights[:E * C].reshape(E, C).cpu().numpy()

    @property
    def bias(self):
        return self.weights[self.embed_size * self.num_classes:].cpu().numpy()


# ---- host-side validation ------------------------------------------------------------------------------------------------------
def _check_emb(emb, need_device=True):
    import torch
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous() or emb.shape[0] < 1:
        raise ValueError("emb must be a contiguous float32 tensor of shape (N, E), N >= 1")
    N, E = int(emb.shape[0]), int(emb.shape[1])
    if max_classes(E) == 0:
        raise ValueError("E = %d: the embedding width must be a multiple of 4 in 4..128" % E)
    if need_device and not emb.is_cuda:
        raise ValueError("emb must live on the GPU (kws_amd.transfer.embed returns it there)")
    return N, E


def _host_labels(y, N):
    import torch
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    y = y.reshape(-1)
    if y.shape[0] != N:
        raise ValueError("%d labels for %d embeddings" % (y.shape[0], N))
    if y.dtype.kind not in "iu":
        raise ValueError("labels must be integers")
    return y.astype(np.int64)


def _check_classes(E, C):
    lim = max_classes(E)
    if C < 2 or C > lim:
        raise ValueError("num_classes = %d: a head on %d-wide embeddings takes 2..%d classes" % (C, E, lim))


def _check_labels(y, C, ignore_index, rows=None):
    ys = y if rows is None else y[rows]
    bad = (ys < 0) | (ys >= C)
    if ignore_index and ignore_index > 0:
        bad &= ys != ignore_index
    if bad.any():
        raise ValueError("labels outside [0, %d): %s" % (C, np.unique(ys[bad])[:8].tolist()))


def _check_order(order, N):
    order = np.asarray(order)
    if order.ndim != 1 or order.dtype.kind not in "iu":
        raise ValueError("order must be a 1-D integer array of row numbers")
    if order.size and (order.min() < 0 or order.max() >= N):
        raise ValueError("order entries outside [0, %d)" % N)
    return order.astype(np.int32)


def _optimizer_kind(name):
    if name not in ("adam", "sgd"):
        raise ValueError("optimizer must be 'adam' or 'sgd', not %r (rmsprop, clipping and weight averaging are not built for heads)" % (name,))
    return _l.OPT_KINDS[name]


# ---- one launch --------------------------------------------------------------------------------------------------------------------
def _job_defaults(job):
    j = dict(batch_size=32, optimizer="adam", lr=1e-3, momentum=0.0, class_weights=None, ignore_index=0, init=None, state=None, seed=None)
    j.update(ADAM_DEFAULTS)
    unknown = set(job) - set(j) - {"order", "num_classes"}
    if unknown:
        raise ValueError("unknown job keys %s" % sorted(unknown))
    j.update(job)
    return j


def fit_heads(emb, y, jobs):
    """Trains len(jobs) independent heads in ONE kws_head_fit launch.  emb (N, E) float32 on the GPU, y (N) integer labels, shared by all
    jobs.  A job is a dict: order (row numbers into emb, walked in steps of batch_size; repeats allowed), num_classes, and optionally
    batch_size (32), optimizer ('adam' / 'sgd'), lr, momentum, beta1, beta2, eps, class_weights (C), ignore_index, init (a HeadFit or
    (kernel, bias); None: glorot_uniform from `seed`), state (HeadFit.state of an earlier call).  -> [HeadFit], each with ONE entry in
    loss / accuracy (of this launch; NaN for an empty order)."""
    import torch
    N, E = _check_emb(emb, need_device=False)
    yh = _host_labels(y, N)
    if len(jobs) < 1:
        raise ValueError("no jobs")
    js, orders, cws = [], [], []
    for job in jobs:
        j = _job_defaults(job)
        C = int(j["num_classes"])
        _check_classes(E, C)
        order = _check_order(j["order"], N)
        _check_labels(yh, C, int(j["ignore_index"] or 0), order)
        if int(j["batch_size"]) < 1:
            raise ValueError("batch_size must be >= 1")
        if not 0.0 <= float(j["momentum"]) <= 1.0:
            raise ValueError("momentum must be in [0, 1]")
        j["kind"] = _optimizer_kind(j["optimizer"])
        if j["class_weights"] is not None:
            cw = np.asarray(j["class_weights"], np.float32).reshape(-1)
            if cw.shape[0] != C:
                raise ValueError("%d class weights for %d classes" % (cw.shape[0], C))
            j["class_weights"] = cw
        st = j["state"]
        if st is not None and st["optimizer"] != j["optimizer"]:
            raise ValueError("the carried state belongs to %r, the job asks %r" % (st["optimizer"], j["optimizer"]))
        j["order"] = order
        js.append(j)
    _check_emb(emb, need_device=True)
    dev = emb.device
    # shared arrays: every job's slice of order / class weights / weights, one after the other
    sizes = [(E + 1) * int(j["num_classes"]) for j in js]
    woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    W = torch.empty((int(woff[-1]),), dtype=torch.float32, device=dev)
    M, V = torch.zeros_like(W), torch.zeros_like(W)
    recs = (_l.KwsHeadJob * len(js))()
    ooff = cwoff = 0
    for i, j in enumerate(js):
        C, lo, hi = int(j["num_classes"]), int(woff[i]), int(woff[i + 1])
        init = j["init"]
        if isinstance(init, HeadFit):
            if (init.embed_size, init.num_classes) != (E, C):
                raise ValueError("init is a head of shape (%d, %d), the job is (%d, %d)" % (init.embed_size, init.num_classes, E, C))
            W[lo:hi].copy_(init.weights)
        else:
            k, b = glorot_head(E, C, j["seed"]) if init is None else (np.asarray(init[0], np.float32), np.asarray(init[1], np.float32))
            if k.shape != (E, C) or b.shape != (C,):
                raise ValueError("init must be (kernel (%d, %d), bias (%d,))" % (E, C, C))
            W[lo:hi].copy_(torch.from_numpy(np.concatenate([k.reshape(-1), b])))
        st = j["state"]
        if st is not None:
            for slot, buf in (("m", M), ("v", V)):
                if st.get(slot) is not None:
                    if st[slot].numel() != hi - lo:
                        raise ValueError("the carried state does not have the head's shape")
                    buf[lo:hi].copy_(st[slot])
        r = recs[i]
        r.order_offset, r.weight_offset, r.n_order = ooff, lo, int(j["order"].shape[0])
        r.class_weight_offset = cwoff if j["class_weights"] is not None else -1
        r.t0 = int(st["t"]) if st is not None else 0
        r.batch, r.num_classes, r.ignore_index, r.optimizer = int(j["batch_size"]), C, int(j["ignore_index"] or 0), j["kind"]
        r.lr, r.beta1, r.beta2, r.eps, r.momentum = float(j["lr"]), float(j["beta1"]), float(j["beta2"]), float(j["eps"]), float(j["momentum"])
        orders.append(j["order"])
        ooff += r.n_order
        if j["class_weights"] is not None:
            cws.append(j["class_weights"])
            cwoff += C
    order_d = torch.from_numpy(np.concatenate(orders + [np.zeros((1,), np.int32)])).to(dev)
    cw_d = torch.from_numpy(np.concatenate(cws)).to(dev) if cws else None
    y_d = torch.from_numpy(yh.astype(np.int32)).to(dev)
    stats = torch.zeros((len(js), 2), dtype=torch.float32, device=dev)
    jobs_dev = torch.empty((ctypes.sizeof(recs),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.get_lib().kws_head_fit(emb.data_ptr(), y_d.data_ptr(), N, E, order_d.data_ptr(), cw_d.data_ptr() if cw_d is not None else None,
                                           recs, jobs_dev.data_ptr(), len(js), W.data_ptr(), M.data_ptr(), V.data_ptr(), stats.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    st_h = stats.cpu().numpy().astype(np.float64)           # the one synchronisation of the call
    out = []
    for i, j in enumerate(js):
        lo, hi, n = int(woff[i]), int(woff[i + 1]), int(recs[i].n_order)
        steps = -(-n // int(j["batch_size"]))
        state = dict(optimizer=j["optimizer"], t=int(recs[i].t0) + steps, m=M[lo:hi].clone(), v=V[lo:hi].clone())
        out.append(HeadFit(j["num_classes"], E, W[lo:hi].clone(), state, [st_h[i, 0] / n if n else float("nan")],
                           [st_h[i, 1] / n if n else float("nan")]))
    return out


# ---- epochs ------------------------------------------------------------------------------------------------------------------------
def _lr_of(lr, epoch, epochs):
    if callable(lr):
        return float(lr(epoch))
    if np.ndim(lr) == 0:
        return float(lr)
    if len(lr) != epochs:
        raise ValueError("%d learning rates for %d epochs" % (len(lr), epochs))
    return float(lr[epoch])


def epoch_orders(rows, epochs, seed):
    """the `order` of every epoch: a seeded numpy permutation of `rows` per epoch (np.random.default_rng(seed), drawn in epoch order)"""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows)
    return [rows[rng.permutation(rows.shape[0])] for _ in range(epochs)]


def _fit_epochs(emb, y, specs, epochs):
    """one fit_heads launch per epoch over all of `specs`, carrying weights and optimizer state; -> [HeadFit] with per-epoch loss / accuracy"""
    N, E = _check_emb(emb, need_device=False)
    if epochs < 1:
        raise ValueError("epochs must be >= 1")
    for s in specs:
        s["orders"] = epoch_orders(np.arange(N) if s["rows"] is None else _check_order(s["rows"], N), epochs, s["seed"])
        s["lrs"] = [_lr_of(s["lr"], e, epochs) for e in range(epochs)]
    heads = [None] * len(specs)
    hist = [([], []) for _ in specs]
    for e in range(epochs):
        jobs = []
        for s, h in zip(specs, heads):
            job = {k: v for k, v in s.items() if k not in ("rows", "orders", "lrs", "lr")}
            job.update(order=s["orders"][e], lr=s["lrs"][e])
            if h is not None:
                job.update(init=h, state=h.state)
            jobs.append(job)
        heads = fit_heads(emb, y, jobs)
        for h, (ls, ac) in zip(heads, hist):
            ls.extend(h.loss)
            ac.extend(h.accuracy)
    for h, (ls, ac) in zip(heads, hist):
        h.loss, h.accuracy = ls, ac
    return heads


def fit_head(emb, y, num_classes, epochs=10, batch_size=32, optimizer="adam", lr=1e-3, momentum=0.0, class_weights=None, ignore_index=0,
             seed=0, init=None, state=None, rows=None, beta1=0.9, beta2=0.999, eps=1e-7):
    """Fits Dense(E -> num_classes, softmax) on emb (N, E) / y (N).  Every epoch walks a seeded permutation of the rows (all of them, or
    `rows`) in steps of batch_size -- the last step takes the rest, as Keras does -- in one launch of its own, so lr may be a number, a
    list with one value per epoch or a function of the epoch; the optimizer state is carried on the device and nothing waits for the
    host but the epoch's two statistics.  init: None (glorot_uniform kernel, zero bias, drawn from `seed`), (kernel, bias) or a HeadFit;
    state: HeadFit.state to continue an earlier fit (Adam's step count included).  -> HeadFit."""
    spec = dict(num_classes=int(num_classes), batch_size=int(batch_size), optimizer=optimizer, lr=lr, momentum=momentum,
                class_weights=class_weights, ignore_index=ignore_index, seed=seed, init=init, state=state, rows=rows, beta1=beta1,
                beta2=beta2, eps=eps)
    return _fit_epochs(emb, y, [spec], int(epochs))[0]


class CrossValidation(object):
    """folds: [(train_rows, test_rows)]; seeds: the fit_head seed of every fold; heads: the fold's HeadFit; accuracy / loss: of the held-out rows"""

    def __init__(self, folds, seeds, heads, accuracy, loss):
        self.folds, self.seeds, self.heads, self.accuracy, self.loss = folds, seeds, heads, accuracy, loss


def cross_validate(emb, y, num_classes, folds=5, seed=0, **fit):
    """K-fold cross-validation of a head: the rows are dealt to `folds` parts by a seeded permutation, fold f trains on the others --
    all folds in the same launches (fit_heads), fold f exactly as fit_head(emb, y, num_classes, rows=train_rows, seed=seed + 1 + f, **fit)
    would -- and is scored on its own part (torch: a matrix product and an arg-max, plumbing).  -> CrossValidation."""
    import torch
    N, E = _check_emb(emb, need_device=False)
    folds = int(folds)
    if folds < 2 or folds > N:
        raise ValueError("folds must be in 2..N")
    epochs = int(fit.pop("epochs", 10))
    yh = _host_labels(y, N)
    parts = np.array_split(np.random.default_rng(seed).permutation(N), folds)
    split = [(np.sort(np.concatenate([p for g, p in enumerate(parts) if g != f])), np.sort(parts[f])) for f in range(folds)]
    seeds = [int(seed) + 1 + f for f in range(folds)]
    base = dict(batch_size=32, optimizer="adam", lr=1e-3, momentum=0.0, class_weights=None, ignore_index=0, init=None, state=None)
    base.update(ADAM_DEFAULTS)
    unknown = set(fit) - set(base)
    if unknown:
        raise ValueError("unknown arguments %s" % sorted(unknown))
    base.update(fit)
    specs = [dict(base, num_classes=int(num_classes), rows=tr, seed=s) for (tr, _), s in zip(split, seeds)]
    heads = _fit_epochs(emb, y, specs, epochs)
    y_d = torch.from_numpy(yh).to(emb.device)
    acc, loss = [], []
    for h, (_, te) in zip(heads, split):
        te_d = torch.from_numpy(te).to(emb.device)
        Ek = h.embed_size * h.num_classes
        logits = emb.index_select(0, te_d).double() @ h.weights[:Ek].reshape(h.embed_size, h.num_classes).double() + h.weights[Ek:].double()
        yt = y_d.index_select(0, te_d)
        acc.append(float((logits.argmax(1) == yt).double().mean().item()))
        loss.append(float(torch.nn.functional.cross_entropy(logits, yt).item()))
    return CrossValidation(split, seeds, heads, acc, loss)


# ---- the backbone on both sides ----------------------------------------------------------------------------------------------------
def embed(model, x, batch_size=4096, sample_lengths=None, augment=None, feature_mask=None, step=0):
    """(N, E) float32 on the GPU: what `model`'s score_predict reads in inference mode.  x: whatever model.predict takes, features
    (N, n_features, feature_size[, 1]) or raw audio (N, samples).  The optional arguments are KWSModel.fit's input pipeline, for
    embeddings of an AUGMENTED pass over the clips: sample_lengths (N) and augment (kws_amd.augment.WaveAugment) need raw audio,
    feature_mask (kws_amd.augment.FeatureMask) works on either; clip i is drawn for (`step`, position i).  x itself is never written."""
    import torch
    dm = model._device()
    xd, is_audio = model._to_device_inputs(x)
    n = xd.shape[0]
    if (augment is not None or sample_lengths is not None) and not is_audio:
        raise ValueError("augment / sample_lengths need raw audio (N, samples) input, got features")
    lens_d = None
    if sample_lengths is not None:
        lens_d = sample_lengths if isinstance(sample_lengths, torch.Tensor) else torch.from_numpy(np.asarray(sample_lengths))
        lens_d = lens_d.reshape(-1).to(torch.int32).to(xd.device).contiguous()
        if lens_d.numel() != n:
            raise ValueError("%d sample lengths for %d clips" % (lens_d.numel(), n))
    batch_size = int(batch_size or 4096)
    out = []
    for i in range(0, n, batch_size):
        if augment is not None or lens_d is not None:
            idx = torch.arange(i, min(i + batch_size, n), dtype=torch.int32, device=xd.device)
            feat = model._get_featurizer()(xd, valid_len=lens_d, index=idx, augment=augment, step=step, position_base=i)
        else:
            feat = model._features_of(xd[i:i + batch_size], is_audio).contiguous()
        if feature_mask is not None:
            feat = feature_mask(feat, step=step, position_base=i)          # a new tensor: cached features are a view of x
        out.append(dm.embed(feat))
    if not out:
        return torch.zeros((0, dm.embed_size), dtype=torch.float32, device=dm.device)
    return torch.cat(out)


def set_head(model, head):
    """writes the fitted head into `model` (of head.num_classes classes) in place; every other weight keeps its bits"""
    old = model.get_weights()
    if tuple(old[-2].shape) != (head.embed_size, head.num_classes):
        raise ValueError("the head is %d -> %d, %s's score_predict is %d -> %d"
                         % ((head.embed_size, head.num_classes, model.model_type) + tuple(old[-2].shape)))
    model.set_weights(old[:-2] + [head.kernel, head.bias])
    return model


def with_head(model, head):
    """A new KWSModel of head.num_classes classes: `model`'s backbone weights (and BatchNormalization statistics) under the fitted head.
    It is an ordinary model: predict / evaluate / evaluate_scores / quantize / save and the streaming classes take it as it is."""
    from classifier.model import KWSModel
    old = model.get_weights()
    E = int(old[-2].shape[0])
    if head.embed_size != E:
        raise ValueError("the head reads %d-wide embeddings, %s produces %d" % (head.embed_size, model.model_type, E))
    new = KWSModel(model.model_type, head.num_classes, batch_size=model.batch_size, num_layers=model.num_layers)
    new.set_weights(old[:-2] + [head.kernel, head.bias])
    return new


def fit_frozen(model, x, y, batch_size=32, epochs=1, validation_data=None, callbacks=None, sample_lengths=None, augment=None,
               feature_mask=None, seed=0, verbose=1, init=None):
    """train.py --freeze_backbone: KWSModel.fit's epoch loop with every weight but score_predict frozen.  `model` is compiled (adam or
    sgd without clipping, nesterov or averaging; the loss gives the class weights and ignore_index).  The embeddings of x are computed
    once -- or once per epoch through the input pipeline when augment / feature_mask draw per step -- and each epoch is ONE fit_head launch
    at the optimizer's learning rate at the epoch's start (a decay schedule advances per epoch), with the optimizer state carried on the
    device.  After every epoch the head is written into `model`, which is validated and handed to the callbacks as in fit.
    init: None starts a fresh head (glorot_uniform kernel, zero bias, drawn from `seed`, as fit_head does); 'model' continues from the
    score_predict `model` holds.  Epoch e walks the permutation of seed + e.  -> History.  model.head_fit keeps the last HeadFit."""
    import time
    from classifier.loss import WeightedSparseCategoricalCrossEntropy
    from classifier.model import History
    opt = model.optimizer
    if opt is None or model.loss is None:
        raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")
    if opt.kind not in ("adam", "sgd") or getattr(opt, "average_args", None) is not None or opt.clipvalue or opt.clipnorm or opt.global_clipnorm \
            or getattr(opt, "nesterov", False) or getattr(opt, "amsgrad", False):
        raise ValueError("a frozen backbone trains its head with plain adam or sgd (momentum allowed): no rmsprop, clipping, nesterov, "
                         "amsgrad or weight averaging")
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("a frozen backbone trains its head on one GPU: not under torch.distributed (world > 1)")
    cw = np.asarray(model.loss.weights, np.float32) if isinstance(model.loss, WeightedSparseCategoricalCrossEntropy) else None
    ig = int(model.loss.ignore_index or 0)
    per_epoch = augment is not None or feature_mask is not None
    kw = dict(sample_lengths=sample_lengths, augment=augment, feature_mask=feature_mask)
    emb = None if per_epoch else embed(model, x, **kw)
    if init not in (None, 'model'):
        raise ValueError("init must be None (a fresh head) or 'model'")
    w = model.get_weights()
    head = None
    init, state = (w[-2], w[-1]) if init == 'model' else glorot_head(w[-2].shape[0], model.num_classes, seed), None
    callbacks = list(callbacks or [])
    for cb in callbacks:
        cb.set_model(model)
        cb.on_train_begin()
    model.history = History()
    model.stop_training = False
    n = len(x)
    steps = max(1, -(-n // int(batch_size)))
    fit_kw = dict(batch_size=batch_size, optimizer=opt.kind, momentum=float(getattr(opt, "momentum", 0.0) or 0.0), class_weights=cw,
                  ignore_index=ig)
    if opt.kind == "adam":
        fit_kw.update(beta1=opt.beta_1, beta2=opt.beta_2, eps=opt.epsilon)
    for epoch in range(epochs):
        for cb in callbacks:
            cb.on_epoch_begin(epoch)
        t0 = time.time()
        if per_epoch:
            emb = embed(model, x, step=epoch + 1, **kw)
        lr = opt.current_lr()
        head = fit_head(emb, y, model.num_classes, epochs=1, lr=lr, seed=int(seed) + epoch, init=init, state=state, **fit_kw)
        init, state = head, head.state
        opt.iterations += steps
        set_head(model, head)
        dt = time.time() - t0
        logs = {'loss': float(head.loss[0]), 'accuracy': float(head.accuracy[0])}
        if validation_data is not None:
            logs['val_loss'], logs['val_accuracy'] = model.evaluate(validation_data[0], validation_data[1], batch_size=4096, verbose=0)
        logs['lr'] = lr
        logs['clips_per_sec'] = float(n / dt) if dt > 0 else 0.0
        if verbose:
            print('Epoch %d/%d - %.1fs - %s' % (epoch + 1, epochs, dt, ' - '.join(
                '%s: %.4f' % (k, v) for k, v in logs.items() if k not in ('lr', 'clips_per_sec'))))
        model.history.append(epoch, logs)
        for cb in callbacks:
            cb.on_epoch_end(epoch, logs)
        if model.stop_training:
            break
    for cb in callbacks:
        cb.on_train_end()
    model.head_fit = head
    return model.history


# ---- a bank of heads on one backbone (include/kws.h: kws_heads_apply) ------------------------------------------
def plan_bank(classes, E):
    """Where the heads of a bank lie.  classes: the class count (or the room, for a slot that may take any head up to it) of every
    head.  -> (offsets, count): int64 offsets in floats into the weights array, each a multiple of 4 -- head h takes (E + 1) * classes[h]
    floats, kernel (E, C) row-major then bias (C), kws_head_fit's layout -- and the length of that array.  Host only."""
    E = int(E)
    if E < 4 or E > 128 or E % 4:
        raise ValueError("E = %d: the embedding width must be a multiple of 4 in 4..128" % E)
    classes = np.asarray(classes, np.int64).reshape(-1)
    if classes.size and (classes.min() < 2 or classes.max() > _l.HEADS_MAX_CLASSES):
        raise ValueError("a banked head has 2..%d classes" % _l.HEADS_MAX_CLASSES)
    room = ((E + 1) * classes + 3) // 4 * 4
    offsets = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64) if classes.size else np.zeros((0,), np.int64)
    return offsets, int(room.sum())


def _head_arrays(head, E):
    """a HeadFit or (kernel, bias) -> (C, flat weights: a device tensor for a HeadFit, else a float32 ndarray)"""
    if isinstance(head, HeadFit):
        if head.embed_size != E:
            raise ValueError("the head reads %d-wide embeddings, the bank holds %d-wide ones" % (head.embed_size, E))
        return head.num_classes, head.weights
    k, b = np.asarray(head[0], np.float32), np.asarray(head[1], np.float32)
    if k.ndim != 2 or k.shape[0] != E or b.shape != (k.shape[1],):
        raise ValueError("a head is (kernel (%d, C), bias (C,)), got %s and %s" % (E, k.shape, b.shape))
    return int(k.shape[1]), np.concatenate([k.reshape(-1), b])


class HeadBank(object):
    """`capacity` slots for Dense(embed_size -> C, softmax) heads of up to max_classes classes, resident on the device, that
    kws_heads_apply applies row by row: a keyword set per stream (kws_amd.stream: StreamServer / StreamBatch / scan take `heads=bank`)
    or per fold (score_heads).  weights, head_offset, head_classes: the device tensors of include/kws.h, every slot with room for
    max_classes classes (plan_bank), so any head that fits the bank fits any slot; classes (host mirror, 0: empty) and class_names per slot.
    set / remove are stream-ordered copies and fills: a head is replaced between two pushes of a running server without stopping it.
    device: None is the current HIP device; 'cpu' keeps the arrays in host memory for bookkeeping alone (save / load / planning) --
    nothing is ever applied there, launch refuses embeddings that are not on the GPU."""

    def __init__(self, embed_size, capacity, max_classes, device=None):
        self.embed_size, self.capacity, self.max_classes = int(embed_size), int(capacity), int(max_classes)
        if self.capacity < 1:
            raise ValueError("a bank has at least one slot")
        if not 2 <= self.max_classes <= _l.HEADS_MAX_CLASSES:
            raise ValueError("max_classes = %d is outside 2..%d" % (self.max_classes, _l.HEADS_MAX_CLASSES))
        self.offsets, self.count = plan_bank([self.max_classes] * self.capacity, self.embed_size)
        self.classes = np.zeros((self.capacity,), np.int32)
        self.class_names = [None] * self.capacity
        self.names = [None] * self.capacity                      # an optional name per head (listen.py --head_map refers to it)
        import torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.weights = torch.zeros((self.count,), dtype=torch.float32, device=self.device)
        self.head_offset = torch.from_numpy(self.offsets).to(self.device)
        self.head_classes = torch.zeros((self.capacity,), dtype=torch.int32, device=self.device)

    def __len__(self):
        return int((self.classes > 0).sum())

    def _slot(self, h):
        if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, np.integer)) or not 0 <= h < self.capacity:
            raise ValueError("head id %r is outside 0..%d" % (h, self.capacity - 1))
        return int(h)

    def set(self, h, head, class_names=None, name=None):
        """copies `head` (a HeadFit or (kernel, bias)) into slot h, replacing what was there; class_names: its C names, class 0 the
        background as the servers require; name: the head's own (a user, a keyword set).  Enqueued on the current stream."""
        import torch
        h = self._slot(h)
        C, flat = _head_arrays(head, self.embed_size)
        if C < 2 or C > self.max_classes:
            raise ValueError("a head of %d classes in a bank of 2..%d" % (C, self.max_classes))
        if class_names is not None:
            class_names = list(class_names)
            if len(class_names) != C:
                raise ValueError("%d class names for %d classes" % (len(class_names), C))
            if class_names[0] != 'background':
                raise ValueError("1st class should be background.")
        lo, n = int(self.offsets[h]), (self.embed_size + 1) * C
        with _on(self.device):
            if isinstance(flat, np.ndarray):
                staged = torch.empty((n,), dtype=torch.float32, pin_memory=self.device.type == "cuda")
                staged.numpy()[:] = flat
                self.weights[lo:lo + n].copy_(staged, non_blocking=True)
            else:
                self.weights[lo:lo + n].copy_(flat)
            self.head_classes[h:h + 1].fill_(C)
        self.classes[h], self.class_names[h], self.names[h] = C, class_names, None if name is None else str(name)
        return h

    def add(self, head, class_names=None, name=None):
        """-> the id of the lowest empty slot, now holding `head`"""
        free = np.flatnonzero(self.classes == 0)
        if free.size == 0:
            raise RuntimeError("the bank is full: all %d slots hold a head" % self.capacity)
        return self.set(int(free[0]), head, class_names, name)

    def remove(self, h):
        """empties slot h (classes = 0): rows that name it come out as zeros with pred = -1"""
        import torch
        h = self._slot(h)
        with _on(self.device):
            self.head_classes[h:h + 1].fill_(0)
        self.classes[h], self.class_names[h], self.names[h] = 0, None, None

    def launch(self, emb, R, key, key_stride=1, head_of_key=None, rows=None, want=("probs",)):
        """kws_heads_apply on the current stream.  emb (N, E) float32 CUDA; key: int32 CUDA tensor read at key[r * key_stride];
        head_of_key, rows: int32 CUDA tensors or None.  -> the tensors named in `want`, of 'logits' (R, Cmax), 'probs' (R, Cmax),
        'pred' (R), in that order.  No synchronisation, nothing read back."""
        import torch
        N, E = _check_emb_bank(emb, self)
        unknown = set(want) - {"logits", "probs", "pred"}
        if unknown or not want:
            raise ValueError("want names some of 'logits', 'probs', 'pred', got %r" % (want,))
        R = int(R)
        out = {k: torch.empty((R,) if k == "pred" else (R, self.max_classes), dtype=torch.int32 if k == "pred" else torch.float32,
                              device=emb.device) for k in want}
        ptr = lambda k: out[k].data_ptr() if k in out else None
        with torch.cuda.device(emb.device):
            _l.check(_l.get_lib().kws_heads_apply(emb.data_ptr(), N, E, rows.data_ptr() if rows is not None else None, key.data_ptr(),
                                                  int(key_stride), head_of_key.data_ptr() if head_of_key is not None else None,
                                                  int(head_of_key.numel()) if head_of_key is not None else 0, R, self.weights.data_ptr(),
                                                  self.count, self.head_offset.data_ptr(), self.head_classes.data_ptr(), self.capacity,
                                                  self.max_classes, ptr("logits"), ptr("probs"), ptr("pred"),
                                                  torch.cuda.current_stream().cuda_stream))
        return tuple(out[k] for k in want)

    def apply(self, emb, head, rows=None, want=("probs",)):
        """Row r of the result is head[r] applied to emb[rows[r]] (rows None: emb[r]).  head: (R) head ids, rows: (R) row numbers -- int
        arrays or tensors; an id or row outside the bank / emb, or an empty slot, gives a zero row with pred -1.  -> tuple of `want`."""
        head = _index_tensor(head, emb.device)
        if rows is not None:
            rows = _index_tensor(rows, emb.device)
            if rows.numel() != head.numel():
                raise ValueError("%d rows for %d head ids" % (rows.numel(), head.numel()))
        elif head.numel() > emb.shape[0]:
            raise ValueError("%d head ids for %d embeddings" % (head.numel(), emb.shape[0]))
        return self.launch(emb, head.numel(), head, rows=rows, want=want)

    def save(self, path):
        """the occupied slots' heads and names to a .npz (numpy only on the way back in)"""
        w = self.weights.cpu().numpy()
        data = dict(embed_size=self.embed_size, capacity=self.capacity, max_classes=self.max_classes, classes=self.classes)
        for h in np.flatnonzero(self.classes > 0):
            lo, C = int(self.offsets[h]), int(self.classes[h])
            data["head_%d" % h] = w[lo:lo + (self.embed_size + 1) * C]
            if self.class_names[h] is not None:
                data["names_%d" % h] = np.asarray(self.class_names[h], dtype=str)
            if self.names[h] is not None:
                data["name_%d" % h] = np.asarray(self.names[h], dtype=str)
        with open(path, "wb") as f:
            np.savez(f, **data)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            bank = cls(int(z["embed_size"]), int(z["capacity"]), int(z["max_classes"]), device)
            E = bank.embed_size
            for h in np.flatnonzero(z["classes"] > 0):
                C, flat = int(z["classes"][h]), z["head_%d" % h]
                names = [str(n) for n in z["names_%d" % h]] if "names_%d" % h in z.files else None
                bank.set(int(h), (flat[:E * C].reshape(E, C), flat[E * C:]), names, str(z["name_%d" % h]) if "name_%d" % h in z.files else None)
        return bank

    @classmethod
    def from_fits(cls, heads, names=None, device=None):
        """a bank of exactly these heads (HeadFit or (kernel, bias)), head i in slot i; names: per head its class names, or None"""
        heads = list(heads)
        if not heads:
            raise ValueError("no heads")
        if names is not None and len(names) != len(heads):
            raise ValueError("%d name lists for %d heads" % (len(names), len(heads)))
        E = heads[0].embed_size if isinstance(heads[0], HeadFit) else int(np.asarray(heads[0][0]).shape[0])
        Cs = [h.num_classes if isinstance(h, HeadFit) else int(np.asarray(h[0]).shape[1]) for h in heads]
        if device is None and isinstance(heads[0], HeadFit):
            device = heads[0].weights.device
        bank = cls(E, len(heads), max(Cs), device)
        for i, h in enumerate(heads):
            bank.set(i, h, None if names is None else names[i])
        return bank


def _on(device):
    """the device's context: torch.cuda.device for a GPU, nothing for the host"""
    import contextlib
    import torch
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def _check_emb_bank(emb, bank):
    N, E = int(emb.shape[0]) if emb.dim() == 2 else -1, int(emb.shape[-1])
    import torch
    if emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous() or not emb.is_cuda:
        raise ValueError("emb must be a contiguous float32 CUDA tensor of shape (N, E)")
    if E != bank.embed_size:
        raise ValueError("emb is %d wide, the bank's heads read %d-wide embeddings" % (E, bank.embed_size))
    return N, E


def _index_tensor(a, device):
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError("head ids and row numbers must be integers")
        a = torch.from_numpy(np.ascontiguousarray(a.reshape(-1).astype(np.int32)))
    return a.reshape(-1).to(torch.int32).to(device).contiguous()


def score_heads(emb, y, bank_or_heads, rows_per_head):
    """Every head on its own rows in ONE kws_heads_apply launch: head i (of a HeadBank, or of a list of HeadFit / (kernel, bias) that is
    banked here) is scored on emb[rows_per_head[i]] against y.  -> (accuracy, loss), two lists of floats: the share of rows whose
    arg-max (pred, an exact tie to the lower class) is the label, counted in integers, and the mean of -log p_y over the rows, p the
    kernel's float32 probabilities, summed in float64 by torch.  A head without rows gives NaN twice.  Labels are checked on the host
    (ValueError outside the head's classes)."""
    import torch
    bank = bank_or_heads if isinstance(bank_or_heads, HeadBank) else HeadBank.from_fits(bank_or_heads, device=emb.device)
    N, E = _check_emb_bank(emb, bank)
    yh = _host_labels(y, N)
    if len(rows_per_head) > bank.capacity:
        raise ValueError("%d row sets for a bank of %d heads" % (len(rows_per_head), bank.capacity))
    rows = [_check_order(r, N) for r in rows_per_head]
    for h, r in enumerate(rows):
        if r.size:
            if bank.classes[h] == 0:
                raise ValueError("head %d is empty" % h)
            _check_labels(yh, int(bank.classes[h]), 0, r)
    sizes = np.array([r.size for r in rows], np.int64)
    R = int(sizes.sum())
    nan = float("nan")
    if R == 0:
        return [nan] * len(rows), [nan] * len(rows)
    dev = emb.device
    rows_d = torch.from_numpy(np.concatenate(rows)).to(dev)
    key = torch.repeat_interleave(torch.arange(len(rows), dtype=torch.int32, device=dev), torch.from_numpy(sizes).to(dev), output_size=R)
    yt = torch.from_numpy(yh[np.concatenate(rows)]).to(dev)
    probs, pred = bank.launch(emb, R, key, rows=rows_d, want=("probs", "pred"))
    hit = torch.cumsum((pred.long() == yt).long(), 0)
    nll = torch.cumsum(-torch.log(probs.gather(1, yt.reshape(-1, 1)).reshape(-1).double()), 0)
    ends = torch.from_numpy(np.cumsum(sizes) - 1).to(dev).clamp_(min=0)
    hit_h, nll_h = hit.index_select(0, ends).cpu().numpy(), nll.index_select(0, ends).cpu().numpy()       # the one synchronisation
    acc, loss = [], []
    prev_hit, prev_nll = 0, 0.0
    for h, n in enumerate(sizes):
        if n == 0:
            acc.append(nan)
            loss.append(nan)
            continue
        acc.append(float(int(hit_h[h]) - prev_hit) / float(n))
        loss.append(float(nll_h[h] - prev_nll) / float(n))
        prev_hit, prev_nll = int(hit_h[h]), float(nll_h[h])
    return acc, loss
