"""Case table of the optimizer kernels at their tail, block and partial-sum edges (tests/test_optim_edges_host.py,
tests/test_optim_edges_gpu.py): a hand-made segment table no model produces, driven through the raw C ABI (include/kws.h:
kws_optimizer_step, kws_optimizer_swap, kws_adam_step, kws_sgd_step, kws_rmsprop_step).

csrc/kws_optim.hip cuts every segment into blocks of 1024 floats, one float4 per thread; a thread whose four floats do not all lie in
its block (i + 3 >= end) walks them one by one.  opt_update_kernel then adds up one double per block -- its segment's blocks, or all
of them for the global norm -- 256 at a time.  The table:

    size      blocks   size % 4   there for
    1         1        1          a segment that is nothing but a tail
    2         1        2
    3         1        3
    5         1        1          a float4 and a tail in one block
    1023      1        3          255 float4s, then a tail
    1024      1        0          exactly one block, no tail
    1025      2        1          a second block that holds one float
    2051      3        3          two full blocks, a block of a tail alone
    262145    257      1          256 full blocks and a block of one float: the segment's partial sum takes a second turn of its loop
    263171    258      3          257 full blocks and a tail of 3: the same, with a full block behind the 256th
                                  526 blocks in all: the global sum takes a third turn

Offsets are multiples of 4, at least 8 floats lie between two segments, 4 before the first and at least 4 behind the last.  Everything
here is host-only."""
import collections
import ctypes

import numpy as np

import averaging_ref as ar
from optim_ref import RefOptimizer

CHUNK = 1024                     # csrc/kws_optim.hip kOptChunk
SUM_STRIDE = 256                 # kOptThreads: partial sums added per turn of opt_update_kernel's loop
SIZES = [1, 2, 3, 5, 1023, 1024, 1025, 2051, 262145, 263171]
LEAD, GAP = 4, 8
SENTINEL = 777.25


def _offsets(sizes):
    out, at = [], LEAD
    for n in sizes:
        out.append(at)
        at = (at + n + 3) // 4 * 4 + GAP
    return out, at - GAP + 4


OFFSETS, TOTAL = _offsets(SIZES)
SEGMENTS = list(zip(OFFSETS, SIZES))
BLOCKS = [(n + CHUNK - 1) // CHUNK for n in SIZES]
N_BLOCKS = sum(BLOCKS)
INSIDE = np.zeros((TOTAL,), bool)
for _o, _n in SEGMENTS:
    INSIDE[_o:_o + _n] = True

KINDS = ("sgd", "rmsprop", "adam")
NORMS = ("none", "var", "global")
AVGS = ("none", "blend", "sync")
AVG_MODE = {"none": ar.NONE, "blend": ar.BLEND, "sync": ar.SYNC}
AVG_ALPHA = {"none": 0.0, "blend": 0.3, "sync": 0.5}
LR = {"sgd": 0.05, "rmsprop": 1e-3, "adam": 1e-3}                  # tests/test_optim_gpu.py's
FLAGS_ON = {"sgd": dict(momentum=0.9, nesterov=True), "rmsprop": dict(momentum=0.9, centered=True), "adam": dict(amsgrad=True)}
SLOTS = {"sgd": ("mom",), "rmsprop": ("v", "mg", "mom"), "adam": ("m", "v", "vhat")}      # with every flag on
CLIP = 1.0                       # clipnorm / global_clipnorm: norm-3 segments are clipped, norm-0.3 ones are not
HUGE = 1e20                      # finite in float32; its square is not
HUGE_SEGMENT = 3                 # the 5-float segment
PARAM_RTOL, PARAM_ATOL, SLOT_RTOL, SLOT_ATOL = 1e-5, 1e-6, 1e-5, 1e-6      # tests/test_optim_gpu.py's bounds
FLOAT32_CAP = 0.25               # the float32 restatement stays within a quarter of them: the rest is the device's margin

Case = collections.namedtuple("Case", "label kind norm avg options clipvalue grad_scale steps t0 pattern")


def f32(x):
    return float(np.float32(x))


def plan(offsets, sizes):
    """(the planned workspace as host bytes, n_blocks, the block table as a structured array) through the host-only entry points"""
    from kws_amd import lib as l
    L = l.get_lib()
    o, s = np.asarray(offsets, np.int64), np.asarray(sizes, np.int64)
    po, ps = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for a in (o, s))
    nbytes = int(L.kws_optimizer_workspace_bytes(po, ps, len(o)))
    assert nbytes > 0, L.kws_last_error()
    host = np.zeros((nbytes,), np.uint8)
    nb = ctypes.c_int32()
    l.check(L.kws_optimizer_plan(po, ps, len(o), host.ctypes.data, nbytes, ctypes.byref(nb)))
    tab = np.frombuffer(host[:32 * nb.value].tobytes(), dtype=[("begin", "<i8"), ("end", "<i8"), ("first", "<i4"), ("count", "<i4"),
                                                               ("seg", "<i4"), ("reserved", "<i4")])
    return host, int(nb.value), tab


# ---- gradients --------------------------------------------------------------------------------------------------------
def heavy_part(n):
    """(indices whose entries carry 60 % of a tail_heavy segment's squared norm, their share of that 60 %): the scalar tail (the last
    element where there is none), and for a segment past 256 blocks everything from block 256 on, half of it on the tail"""
    tail = np.arange(n - (n % 4 or 1), n)
    if n <= SUM_STRIDE * CHUNK:
        return tail, np.full(tail.size, 1.0 / tail.size)
    far = np.arange(SUM_STRIDE * CHUNK, n)
    rest = np.setdiff1d(far, tail)
    if rest.size == 0:
        return tail, np.full(tail.size, 1.0 / tail.size)
    return np.concatenate([rest, tail]), np.concatenate([np.full(rest.size, 0.5 / rest.size), np.full(tail.size, 0.5 / tail.size)])


def zero_segment(step):
    """the segment whose gradient is all zeros at this step: the 2-float, the 1025-float and the 262145-float one in turn"""
    return (1, 6, 8)[step % 3]


def gradient(pattern, step, seed=1):
    """the gradient after grad_scale, float32, NaN outside the segments.  Per segment: norm 3 (clipped at 1) or 0.3 (not clipped),
    alternating per segment and step, entries spread over three decades (tests/test_optim_gpu.py: _grads); one segment all zeros.
    tail_heavy moves 60 % of every squared norm onto heavy_part(); huge fills HUGE_SEGMENT with +-1e20 on top of that."""
    rng = np.random.default_rng([seed, step, {"decades": 0, "tail_heavy": 1, "huge": 1}[pattern]])
    g = np.full((TOTAL,), np.nan, np.float32)
    for k, (o, n) in enumerate(SEGMENTS):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-1.5, 1.5, n)
        x /= np.linalg.norm(x)
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        if pattern != "decades":
            idx, share = heavy_part(n)
            body = np.ones(n, bool)
            body[idx] = False
            if body.any():
                x[body] *= np.sqrt(0.4) / np.linalg.norm(x[body])
                x[idx] = sign[idx] * np.sqrt(0.6 * share)
            else:
                x[idx] = sign[idx] * np.sqrt(share)
        x *= 3.0 if (k + step) % 2 == 0 else 0.3
        if k == zero_segment(step):
            x[:] = 0.0
        if pattern == "huge" and k == HUGE_SEGMENT:
            x = sign * HUGE
        g[o:o + n] = x.astype(np.float32)
    return g


_GRADS = {}


def gradients(case):
    """the case's gradients after grad_scale, one per step: drawn once per pattern and shared, never written"""
    out = []
    for s in range(case.steps):
        if (case.pattern, s) not in _GRADS:
            g = gradient(case.pattern, s)
            g.setflags(write=False)
            _GRADS[(case.pattern, s)] = g
        out.append(_GRADS[(case.pattern, s)])
    return out


def raw_gradients(case):
    """what the device is handed: gradient / grad_scale, exact because every grad_scale is a power of two"""
    assert np.log2(case.grad_scale) == int(np.log2(case.grad_scale))
    return [(g / np.float32(case.grad_scale)).astype(np.float32) for g in gradients(case)]


_START = {}


def start(name):
    """initial parameters ('p') and averaging slot ('avg'): standard normal inside the segments, the sentinel outside"""
    if name not in _START:
        rng = np.random.default_rng({"p": 7, "avg": 8}[name])
        x = np.where(INSIDE, rng.standard_normal(TOTAL), SENTINEL).astype(np.float32)
        x.setflags(write=False)
        _START[name] = x
    return _START[name]


# ---- the cases --------------------------------------------------------------------------------------------------------
def _cases():
    cases = []

    def add(label, kind, norm, avg, options=None, clipvalue=0.0, grad_scale=1.0, steps=3, t0=1, pattern=None):
        options = dict(FLAGS_ON[kind]) if options is None else options
        pattern = pattern or ("decades" if norm == "none" else "tail_heavy")
        cases.append(Case(label, kind, norm, avg, tuple(sorted(options.items())), clipvalue, grad_scale, steps, t0, pattern))
    k = 0
    for kind in KINDS:
        for norm in NORMS:
            for avg in AVGS:
                # clipvalue 0.5 leaves the heavy entries of the norm-3 segments clipped and still the larger part of their norm
                add("%s-%s-%s" % (kind, norm, avg), kind, norm, avg, clipvalue=0.5 if k % 2 else 0.0, grad_scale=(1.0, 0.5, 1.0 / 128)[k % 3])
                k += 1
    # beta^t underflows: lr_t is formed on the host, in double
    add("adam-late", "adam", "var", "blend", grad_scale=0.5, t0=10 ** 6)
    # a float32 sum of squares would overflow; value clipping is off, or it would remove the 1e20
    add("sgd-var-huge", "sgd", "var", "none", pattern="huge")
    add("adam-global-huge", "adam", "global", "blend", pattern="huge", grad_scale=0.5)
    # the branches behind the flags, at the tails: no momentum (other formulas, no slot), momentum without nesterov, tail_heavy
    # under clipvalue alone
    add("sgd-plain", "sgd", "var", "blend", options={}, grad_scale=0.5)
    add("sgd-heavy-ball", "sgd", "global", "none", options=dict(momentum=0.5), clipvalue=0.5)
    add("rmsprop-plain", "rmsprop", "var", "sync", options={}, clipvalue=0.5)
    add("rmsprop-centered", "rmsprop", "global", "none", options=dict(centered=True), grad_scale=1.0 / 128)
    add("adam-plain", "adam", "none", "sync", options={}, clipvalue=0.5, pattern="tail_heavy")
    return cases


CASES = _cases()
CASE = {c.label: c for c in CASES}

# what the table is there to run
REQUIRED = {("tail", 1), ("tail", 2), ("tail", 3), "single_float_block", "segment_blocks_above_256", "table_blocks_above_512"} | \
    {("combo", kind, norm, avg) for kind in KINDS for norm in NORMS for avg in AVGS}


def covered():
    """the members of REQUIRED the table and the case list reach, from the sizes and the cases alone"""
    out = set()
    for n in SIZES:
        if n % 4:
            out.add(("tail", n % 4))
        if n % CHUNK == 1 and n > CHUNK:
            out.add("single_float_block")
        if (n + CHUNK - 1) // CHUNK > SUM_STRIDE:
            out.add("segment_blocks_above_256")
    if N_BLOCKS > 2 * SUM_STRIDE:
        out.add("table_blocks_above_512")
    for c in CASES:
        out.add(("combo", c.kind, c.norm, c.avg))
    return out


def slots_of(case):
    """the slots include/kws.h requires for the case; every other one is passed as NULL"""
    o = dict(case.options)
    if case.kind == "adam":
        return ("m", "v") + (("vhat",) if o.get("amsgrad") else ())
    if case.kind == "rmsprop":
        return ("v",) + (("mg",) if o.get("centered") else ()) + (("mom",) if o.get("momentum", 0.0) > 0 else ())
    return ("mom",) if o.get("momentum", 0.0) > 0 else ()


def _make(cls, case):
    o = dict(case.options)
    rho = 0.9 if case.kind == "rmsprop" else 0.999
    opt = cls(case.kind, f32(LR[case.kind]), beta1=f32(0.9), beta2=f32(rho), eps=f32(1e-7), momentum=f32(o.get("momentum", 0.0)),
              nesterov=o.get("nesterov", False), centered=o.get("centered", False), amsgrad=o.get("amsgrad", False),
              clipvalue=f32(case.clipvalue), clipnorm=f32(CLIP if case.norm == "var" else 0.0),
              global_clipnorm=f32(CLIP if case.norm == "global" else 0.0))
    opt.t = case.t0 - 1
    return opt


def run_oracle(case):
    """the float64 oracle over the case: yields (p, avg or None, slots) after every step; the arrays are the running ones"""
    ref = _make(RefOptimizer, case)
    p = start("p").astype(np.float64)
    avg = None if case.avg == "none" else start("avg").astype(np.float64)
    for g in gradients(case):
        ref.step(p, np.where(INSIDE, g, 0.0), SEGMENTS)
        ar.apply(AVG_MODE[case.avg], f32(AVG_ALPHA[case.avg]), p, avg, SEGMENTS)
        yield p, avg, ref.slots


def run_float32(case):
    """the float32 restatement over the case, as run_oracle"""
    opt = _make(Float32Optimizer, case)
    p = start("p").copy()
    avg = None if case.avg == "none" else start("avg").copy()
    for g in raw_gradients(case):
        opt.step(p, np.where(INSIDE, g, np.float32(0.0)), SEGMENTS, case.grad_scale)
        ar.apply(AVG_MODE[case.avg], f32(AVG_ALPHA[case.avg]), p, avg, SEGMENTS, dtype=np.float32)
        yield p, avg, opt.slots


def bound_ratio(got, want, rtol, atol):
    """the worst |got - want| / (atol + rtol |want|) inside the segments: <= 1 is what assert_allclose(rtol, atol) accepts"""
    got, want = np.asarray(got, np.float64)[INSIDE], np.asarray(want, np.float64)[INSIDE]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def slot_atol(want):
    return SLOT_ATOL * max(float(np.abs(want[INSIDE]).max()), 1e-30)


# ---- the device's arithmetic in numpy ---------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64; the sum is rounded to float64 and then to float32 (a double rounding
    that differs from fmaf's single one by at most one float32 ulp, and only at a tie)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


class Float32Optimizer(RefOptimizer):
    """csrc/kws_optim.hip restated: the sums of squares in float64, everything else in float32 with one rounding per operation in the
    kernel's order (update_one; its fused multiply-adds where it spells them out).  step(p, g, segments, grad_scale) takes the raw
    float32 gradient and updates p (float32) in place."""

    def slot(self, name, like):
        if name not in self.slots:
            self.slots[name] = np.zeros_like(like, dtype=np.float32)
        return self.slots[name]

    def transform(self, g, segments, grad_scale=1.0):
        F = np.float32
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ge = np.asarray(g, F) * F(grad_scale)
            if self.clipvalue:
                cv = F(self.clipvalue)
                ge = np.where(ge > cv, cv, np.where(ge < -cv, -cv, ge))           # a NaN stays NaN
            sums = [float(np.sum(ge[o:o + n].astype(np.float64) ** 2)) for o, n in segments]
            if self.clipnorm:
                c = F(self.clipnorm)
                for (o, n), s in zip(segments, sums):
                    sq = F(s)
                    nrm = F(np.sqrt(s)) if sq > 0 else sq
                    den = nrm if nrm != nrm else np.maximum(nrm, c)
                    ge[o:o + n] = ge[o:o + n] * c / den
            if self.global_clipnorm:
                c = F(self.global_clipnorm)
                s = 0.0
                for x in sums:
                    s += x
                nrm = F(np.sqrt(s))
                scale = c * np.minimum(F(1) / nrm, F(1) / c) if np.isfinite(nrm) else F(np.nan)
                for o, n in segments:
                    ge[o:o + n] = ge[o:o + n] * scale
        return ge

    def step(self, p, g, segments, grad_scale=1.0):
        F = np.float32
        self.t += 1
        ge = self.transform(g, segments, grad_scale)
        lr, mu, b1, b2, eps = F(self.lr), F(self.momentum), F(self.beta1), F(self.beta2), F(self.eps)
        one = F(1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.kind == "sgd":
                if mu > 0:
                    mo = self.slot("mom", p)
                    mo[:] = mu * mo - lr * ge
                    p += (mu * mo - lr * ge) if self.nesterov else mo
                else:
                    p[:] = _fma(-lr, ge, p)
            elif self.kind == "rmsprop":
                v = self.slot("v", p)
                v[:] = b2 * v + (one - b2) * ge * ge
                d = v
                if self.centered:
                    mg = self.slot("mg", p)
                    mg[:] = b2 * mg + (one - b2) * ge
                    d = v - mg * mg
                if mu > 0:
                    mo = self.slot("mom", p)
                    mo[:] = mu * mo + lr * ge / np.sqrt(d + eps)
                    p -= mo
                else:
                    p -= lr * ge / (np.sqrt(d) + eps)
            else:
                m, v = self.slot("m", p), self.slot("v", p)
                m[:] = _fma(b1, m, (one - b1) * ge)
                v[:] = _fma((one - b2) * ge, ge, b2 * v)
                lr_t = F(float(lr) * np.sqrt(1.0 - float(b2) ** self.t) / (1.0 - float(b1) ** self.t))   # on the host, in double
                if self.amsgrad:
                    vh = self.slot("vhat", p)
                    vh[:] = np.maximum(vh, v)
                    p -= lr_t * m / (np.sqrt(vh) + eps)
                else:
                    p -= lr_t * m / (np.sqrt(v) + eps)
        return p
