"""GPU tests of the optimizer kernels at their tail, block and partial-sum edges, through the raw C ABI (kws_amd.lib) on the hand-made
table of tests/optim_edge_cases.py: every (kind, norm mode, averaging mode) with every flag on against the float64 oracle after every
step, run-to-run bit identity at 526 blocks, the non-finite norm rules at tail elements, kws_optimizer_swap, and the three plain steps
at sizes that are no multiple of their vector width."""
import ctypes

import numpy as np
import pytest

import averaging_ref as ar
import optim_edge_cases as ec
from optim_ref import RefOptimizer

pytestmark = pytest.mark.gpu

SLOT_NAMES = ("m", "v", "vhat", "mg", "mom")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class _Table(object):
    """a planned segment table on the device and the launch of one kws_optimizer_step over it"""

    def __init__(self, torch, offsets, sizes):
        from kws_amd import lib as l
        self.l, self.L, self.torch = l, l.get_lib(), torch
        host, self.n_blocks, _ = ec.plan(offsets, sizes)
        self.ws_bytes = host.nbytes
        self.ws = torch.from_numpy(host).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream

    def device(self, host):
        return self.torch.from_numpy(np.array(host, np.float32)).cuda()

    def step(self, kind, p, grad, slots, options=(), lr=None, t=1, grad_scale=1.0, clipvalue=0.0, norm="none", avg=None,
             avg_mode=ar.NONE, avg_alpha=0.0):
        """`slots`: name -> device buffer; a slot that is not given is passed as NULL"""
        l, o = self.l, dict(options)
        flags = (l.OPT_NESTEROV if o.get("nesterov") else 0) | (l.OPT_CENTERED if o.get("centered") else 0) | \
            (l.OPT_AMSGRAD if o.get("amsgrad") else 0)
        ptr = {name: (slots[name].data_ptr() if name in slots else None) for name in SLOT_NAMES}
        a = l.KwsOptimizerArgs(kind=l.OPT_KINDS[kind], flags=flags, params=p.data_ptr(), grads=grad.data_ptr(), m=ptr["m"], v=ptr["v"],
                               vhat=ptr["vhat"], mg=ptr["mg"], mom=ptr["mom"], ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes,
                               n_blocks=self.n_blocks, lr=ec.LR[kind] if lr is None else lr, beta1=0.9,
                               beta2=0.9 if kind == "rmsprop" else 0.999, eps=1e-7, momentum=o.get("momentum", 0.0), t=t,
                               grad_scale=grad_scale, clipvalue=clipvalue, clipnorm=ec.CLIP if norm == "var" else 0.0,
                               global_clipnorm=ec.CLIP if norm == "global" else 0.0, avg=None if avg is None else avg.data_ptr(),
                               avg_mode=avg_mode, avg_alpha=avg_alpha)
        l.check(self.L.kws_optimizer_step(ctypes.byref(a), self.stream))


_TABLE = {}


def _edge_table(torch):
    if "edge" not in _TABLE:
        _TABLE["edge"] = _Table(torch, ec.OFFSETS, ec.SIZES)
        assert _TABLE["edge"].n_blocks == ec.N_BLOCKS == 526
    return _TABLE["edge"]


def _slot_start():
    """slots start at zero inside the segments and hold the sentinel outside"""
    return np.where(ec.INSIDE, 0.0, ec.SENTINEL).astype(np.float32)


def _run_case(torch, case, raw=None, steps=None):
    """the case on the device: yields the host copies (p, avg or None, slots) after every step.  Only the buffers include/kws.h
    requires for the case exist; the others are NULL."""
    tab = _edge_table(torch)
    p = tab.device(ec.start("p"))
    avg = None if case.avg == "none" else tab.device(ec.start("avg"))
    slots = {name: tab.device(_slot_start()) for name in ec.slots_of(case)}
    grad = torch.empty_like(p)
    for s, g in enumerate((ec.raw_gradients(case) if raw is None else raw)[:steps]):
        grad.copy_(torch.from_numpy(g))
        tab.step(case.kind, p, grad, slots, case.options, t=case.t0 + s, grad_scale=case.grad_scale, clipvalue=case.clipvalue,
                 norm=case.norm, avg=avg, avg_mode=ec.AVG_MODE[case.avg], avg_alpha=ec.AVG_ALPHA[case.avg])
        yield p.cpu().numpy(), None if avg is None else avg.cpu().numpy(), {k: v.cpu().numpy() for k, v in slots.items()}


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


_RATIOS = {}


def _check_case(torch, case):
    """every step of the case against the float64 oracle at tests/test_optim_gpu.py's bounds; returns the worst error / bound ratios.
    Run once per case."""
    if case.label in _RATIOS:
        return _RATIOS[case.label]
    worst = {"params": 0.0, "slots": 0.0, "avg": 0.0}
    out = ~ec.INSIDE
    ins = ec.INSIDE
    steps = 0
    for (p, avg, slots), (pr, avgr, slotsr) in zip(_run_case(torch, case), ec.run_oracle(case)):
        where = "%s, step %d" % (case.label, steps)
        worst["params"] = max(worst["params"], ec.bound_ratio(p, pr, ec.PARAM_RTOL, ec.PARAM_ATOL))
        np.testing.assert_allclose(p[ins], pr[ins], rtol=ec.PARAM_RTOL, atol=ec.PARAM_ATOL, err_msg="params, " + where)
        assert _same_bits(p[out], ec.start("p")[out]), "params outside the segments, " + where
        assert set(slots) == set(slotsr) == set(ec.slots_of(case))
        for name, want in slotsr.items():
            worst["slots"] = max(worst["slots"], ec.bound_ratio(slots[name], want, ec.SLOT_RTOL, ec.slot_atol(want)))
            np.testing.assert_allclose(slots[name][ins], want[ins], rtol=ec.SLOT_RTOL, atol=ec.slot_atol(want), err_msg=name + ", " + where)
            assert _same_bits(slots[name][out], _slot_start()[out]), name + " outside the segments, " + where
        if avg is not None:
            worst["avg"] = max(worst["avg"], ec.bound_ratio(avg, avgr, ec.SLOT_RTOL, ec.slot_atol(avgr)))
            np.testing.assert_allclose(avg[ins], avgr[ins], rtol=ec.SLOT_RTOL, atol=ec.slot_atol(avgr), err_msg="avg, " + where)
            assert _same_bits(avg[out], ec.start("avg")[out]), "avg outside the segments, " + where
            if case.avg == "sync":
                np.testing.assert_array_equal(p[ins], avg[ins])              # the fast weights restart at the slow ones
        steps += 1
    assert steps == case.steps
    _RATIOS[case.label] = worst
    return worst


@pytest.mark.parametrize("case", ec.CASES, ids=[c.label for c in ec.CASES])
def test_every_case_matches_the_oracle_after_every_step(torch, case):
    worst = _check_case(torch, case)
    print("%s: worst error / bound  params %.3g  slots %.3g  avg %.3g" % (case.label, worst["params"], worst["slots"], worst["avg"]))


def test_worst_ratios_per_kind(torch):
    for kind in ec.KINDS:
        rows = [_check_case(torch, c) for c in ec.CASES if c.kind == kind]
        print("%s: worst error / bound  params %.3g  slots %.3g  avg %.3g" % (kind, max(r["params"] for r in rows),
                                                                              max(r["slots"] for r in rows), max(r["avg"] for r in rows)))
        assert max(max(r.values()) for r in rows) <= 1.0


@pytest.mark.parametrize("label", ["sgd-none-sync", "rmsprop-var-blend", "adam-global-sync"])
def test_two_runs_are_bit_identical_at_526_blocks(torch, label):
    case = ec.CASE[label]
    assert _edge_table(torch).n_blocks == 526
    a, b = list(_run_case(torch, case))[-1], list(_run_case(torch, case))[-1]
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert set(a[2]) == set(b[2]) == set(ec.slots_of(case))
    for name in a[2]:
        assert _same_bits(a[2][name], b[2][name]), name
    assert not _same_bits(a[0], ec.start("p"))


# ---- the non-finite rules of include/kws.h, at tail elements ------------------------------------------------------------------
# (tests/test_optim_edges_host.py works the same rules by hand on the oracle; the expected values here follow from them: a zero
# gradient leaves a parameter's bits and every slot at zero, whatever the kind)
def _one_step(torch, kind, norm, bad_segment, bad):
    case = ec.Case("nonfinite", kind, norm, "none", tuple(sorted(ec.FLAGS_ON[kind].items())), 0.0, 1.0, 1, 1, "tail_heavy")
    g = ec.gradients(case)[0].copy()
    o, n = ec.SEGMENTS[bad_segment]
    assert bad_segment != ec.zero_segment(0) and n % 4 != 0
    at = o + n - 1                                            # the last element: in the scalar tail
    if bad is not None:
        g[at] = bad
    (p, _, slots), = _run_case(torch, case, raw=[g])
    return p, slots, o, n, at


@pytest.mark.parametrize("kind", ec.KINDS)
def test_inf_in_the_tail_of_the_2051_segment_zeroes_its_finite_gradients_only(torch, kind):
    k = ec.SIZES.index(2051)
    clean, clean_slots, o, n, at = _one_step(torch, kind, "var", k, None)
    p, slots, _, _, _ = _one_step(torch, kind, "var", k, np.inf)
    p0 = ec.start("p")
    assert np.isnan(p[at]) and np.isnan(p).sum() == 1
    assert _same_bits(p[o:at], p0[o:at])                      # a zero gradient: the parameters keep their bits
    assert not _same_bits(clean[o:at], p0[o:at])
    other = np.ones(ec.TOTAL, bool)
    other[o:o + n] = False
    assert _same_bits(p[other], clean[other])                 # every other segment, and the padding, as without the inf
    assert _same_bits(p[~ec.INSIDE], p0[~ec.INSIDE])
    for name in ec.SLOTS[kind]:
        assert (slots[name][o:at] == 0).all(), name
        assert _same_bits(slots[name][other], clean_slots[name][other]), name


@pytest.mark.parametrize("kind", ec.KINDS)
def test_nan_in_a_tail_poisons_that_segment_only(torch, kind):
    k = ec.SIZES.index(263171)                                # 258 blocks: every one of them has to see the NaN
    clean, clean_slots, o, n, at = _one_step(torch, kind, "var", k, None)
    p, slots, _, _, _ = _one_step(torch, kind, "var", k, np.nan)
    assert np.isnan(p[o:o + n]).all() and np.isfinite(clean).all()
    other = np.ones(ec.TOTAL, bool)
    other[o:o + n] = False
    assert _same_bits(p[other], clean[other])
    for name in ec.SLOTS[kind]:
        assert _same_bits(slots[name][other], clean_slots[name][other]), name


@pytest.mark.parametrize("kind", ec.KINDS)
def test_inf_in_the_one_float_segment_poisons_everything_under_the_global_norm(torch, kind):
    p, slots, o, n, at = _one_step(torch, kind, "global", 0, np.inf)
    assert n == 1
    assert np.isnan(p[ec.INSIDE]).all()
    assert _same_bits(p[~ec.INSIDE], ec.start("p")[~ec.INSIDE])
    for name in ec.SLOTS[kind]:
        assert _same_bits(slots[name][~ec.INSIDE], _slot_start()[~ec.INSIDE]), name


def test_a_zero_segment_keeps_its_parameters_and_nothing_becomes_nan(torch):
    clean, slots, _, _, _ = _one_step(torch, "sgd", "var", 2, None)
    o, n = ec.SEGMENTS[ec.zero_segment(0)]
    assert np.isfinite(clean).all() and _same_bits(clean[o:o + n], ec.start("p")[o:o + n])
    assert (slots["mom"][o:o + n] == 0).all()


# ---- kws_optimizer_swap --------------------------------------------------------------------------------------------------------
def test_swap_exchanges_the_insides_and_twice_restores_every_bit(torch):
    tab = _edge_table(torch)
    p0 = ec.start("p")
    a0 = np.where(ec.INSIDE, ec.start("avg"), -ec.SENTINEL).astype(np.float32)     # other padding: an exchange there would show
    p, avg = tab.device(p0), tab.device(a0)

    def swap():
        tab.l.check(tab.L.kws_optimizer_swap(p.data_ptr(), avg.data_ptr(), tab.ws.data_ptr(), tab.ws_bytes, tab.n_blocks, tab.stream))
    swap()
    p1, a1 = p.cpu().numpy(), avg.cpu().numpy()
    ins = ec.INSIDE
    assert _same_bits(p1[ins], a0[ins]) and _same_bits(a1[ins], p0[ins])
    assert _same_bits(p1[~ins], p0[~ins]) and _same_bits(a1[~ins], a0[~ins])
    swap()
    assert _same_bits(p.cpu().numpy(), p0) and _same_bits(avg.cpu().numpy(), a0)


# ---- the plain steps: adam_kernel runs float4s and a scalar tail, sgd_kernel / rmsprop_kernel one float per thread ------------
PLAIN_SIZES = {"adam": (1, 2, 3, 5, 1023, 1025), "sgd": (1, 255, 257, 1025), "rmsprop": (1, 255, 257, 1025)}
PLAIN_STEPS = 3
PLAIN_SCALE = 0.5


def _plain_inputs(n):
    """(padded length, initial parameters, raw gradients): the sentinel / NaN in the floats after n"""
    total = (n + 3) // 4 * 4 + 8
    rng = np.random.default_rng(100 + n)
    inside = np.arange(total) < n
    p0 = np.where(inside, rng.standard_normal(total), ec.SENTINEL).astype(np.float32)
    grads = []
    for s in range(PLAIN_STEPS):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-1.5, 1.5, n)
        g = np.full((total,), np.nan, np.float32)
        g[:n] = (x * (3.0 if s % 2 == 0 else 0.3) / np.linalg.norm(x)).astype(np.float32)
        grads.append(g)
    return total, inside, p0, grads


@pytest.mark.parametrize("kind,n", [(k, n) for k in ("adam", "sgd", "rmsprop") for n in PLAIN_SIZES[k]])
def test_plain_steps_at_their_edges(torch, kind, n):
    """kws_adam_step / kws_sgd_step / kws_rmsprop_step on n floats against the oracle, the floats after n untouched, and
    kws_optimizer_step with default options on the one-segment table [0, n) giving the same bits"""
    total, inside, p0, grads = _plain_inputs(n)
    tab = _Table(torch, [0], [n])
    assert tab.n_blocks == (n + 1023) // 1024
    L, l, stream = tab.L, tab.l, tab.stream
    lr, b1, b2, eps = ec.LR[kind], 0.9, 0.9 if kind == "rmsprop" else 0.999, 1e-7
    names = {"adam": ("m", "v"), "sgd": (), "rmsprop": ("v",)}[kind]
    slot0 = np.where(inside, 0.0, ec.SENTINEL).astype(np.float32)
    plain = dict(p=tab.device(p0), **{k: tab.device(slot0) for k in names})
    fused = dict(p=tab.device(p0), **{k: tab.device(slot0) for k in names})
    grad = torch.empty_like(plain["p"])
    ref = RefOptimizer(kind, ec.f32(lr), beta1=ec.f32(b1), beta2=ec.f32(b2), eps=ec.f32(eps))
    pr = p0.astype(np.float64)
    worst = 0.0
    for s, g in enumerate(grads):
        grad.copy_(torch.from_numpy(g / np.float32(PLAIN_SCALE)))
        if kind == "adam":
            l.check(L.kws_adam_step(plain["p"].data_ptr(), grad.data_ptr(), plain["m"].data_ptr(), plain["v"].data_ptr(), n, lr, b1, b2,
                                    eps, s + 1, PLAIN_SCALE, stream))
        elif kind == "sgd":
            l.check(L.kws_sgd_step(plain["p"].data_ptr(), grad.data_ptr(), n, lr, PLAIN_SCALE, stream))
        else:
            l.check(L.kws_rmsprop_step(plain["p"].data_ptr(), grad.data_ptr(), plain["v"].data_ptr(), n, lr, b2, eps, PLAIN_SCALE, stream))
        tab.step(kind, fused["p"], grad, {k: fused[k] for k in names}, t=s + 1, grad_scale=PLAIN_SCALE)
        ref.step(pr, np.where(inside, g, 0.0), [(0, n)])
        got = {k: v.cpu().numpy() for k, v in plain.items()}
        np.testing.assert_allclose(got["p"][:n], pr[:n], rtol=ec.PARAM_RTOL, atol=ec.PARAM_ATOL, err_msg="params, step %d" % s)
        worst = max(worst, float((np.abs(got["p"][:n] - pr[:n]) / (ec.PARAM_ATOL + ec.PARAM_RTOL * np.abs(pr[:n]))).max()))
        assert _same_bits(got["p"][n:], p0[n:])
        assert set(ref.slots) == set(names)
        for name in names:
            want = ref.slots[name][:n]
            atol = ec.SLOT_ATOL * max(float(np.abs(want).max()), 1e-30)
            assert np.abs(want).max() > 0
            np.testing.assert_allclose(got[name][:n], want, rtol=ec.SLOT_RTOL, atol=atol, err_msg="%s, step %d" % (name, s))
            worst = max(worst, float((np.abs(got[name][:n] - want) / (atol + ec.SLOT_RTOL * np.abs(want))).max()))
            assert _same_bits(got[name][n:], slot0[n:]), name
        for name in ("p",) + names:
            assert _same_bits(fused[name].cpu().numpy(), got[name]), "%s, step %d: kws_optimizer_step differs from the plain step" % (name, s)
    print("%s n=%d: worst error / bound %.3g" % (kind, n, worst))
