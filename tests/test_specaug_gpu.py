"""GPU tests of the feature-mask stage (include/kws.h: kws_feature_mask; kws_amd.augment.FeatureMask) against the numpy restatement of
tests/specaug_ref.py: bit equality outside the masks, exact zeros, the mean fill and the warp within their float32 bounds, the edges
through explicit plans, determinism and sharding.  Inputs have the magnitude of MFCC features (uniform in [-60, 20]): the bounds scale
with max|x|.

The bounds.  u = 2^-24 is the float32 unit roundoff.
  warp: y = (1 - fr) a + fr b from the float32 weight fr that the reference takes as well: one rounding for 1 - fr, two products, one sum.
        Each of the four roundings is relative to a quantity of at most |a| + |b| (the weights are in [0, 1]), so
        |y - y_ref| <= 4 u (|a| + |b|), a = x[k], b = x[k + 1].
  mean: the float32 sum of T terms in a fixed order and its division by T: the partial sums are at most T max|y|, T - 1 additions and one
        division err at most T u (T max|y|) / T = T u max|y|; every warped term y[t] carries its own 4 u (|a| + |b|) <= 8 u max|x|, and
        the mean of those is at most 8 u max|x|; max|y| <= max|x| (y interpolates).  Together (T + 8) u max|x| per clip."""
import numpy as np
import pytest

import specaug_ref as sa

pytestmark = pytest.mark.gpu

U = sa.U
SHAPES = [(30, 20), (30, 40), (7, 13), (124, 40)]           # (30, 40): use_delta; (7, 13): 91 floats per clip, the scalar path
BATCHES = [1, 3, 5, 67]                                     # less than a block, one over a block, an odd tail
STEP, SEED = 11, 4


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _feats(B, T, F, seed=0):
    return np.random.default_rng(seed).uniform(-60.0, 20.0, (B, T, F)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """two arrays (or scalars) of plan records, byte for byte"""
    return np.ascontiguousarray(a, sa.DTYPE).tobytes() == np.ascontiguousarray(b, sa.DTYPE).tobytes()


def _run(torch, fm, x, step=STEP, base=0, in_place=False, plan=None):
    """-> (out, records): one call of the stage on x (numpy), in place on the device copy or into a new tensor"""
    from kws_amd.augment import mask_records
    xd = torch.from_numpy(x).cuda()
    keep = xd.clone()
    out, pl = fm(xd, step, position_base=base, out=xd if in_place else None, plan=plan, return_plan=True)
    torch.cuda.synchronize()
    if in_place:
        assert out.data_ptr() == xd.data_ptr()
    else:
        assert torch.equal(xd, keep), "the input changed in an out-of-place call"
    return out.cpu().numpy(), mask_records(pl)


def _base_for(B, T, F, rate):
    """the first position_base whose B reference plans make the test mean something: decided on the reference alone"""
    for base in range(4096):
        r = sa.np_draws(SEED ^ sa.MIX, STEP, base + np.arange(B), T, F, rate)
        on = r["apply"] == 1
        if not on.any() or (B >= 3 and on.all()):
            continue
        if 2 * (r["tw"][on].max(1) > 0).sum() >= on.sum() and 2 * (r["fw"][on].max(1) > 0).sum() >= on.sum():
            return base
    raise AssertionError("no position base found")


def _check(out, x, recs, fill, what):
    """every clip against the restatement -> (worst mean error / its bound, worst warp error / its bound)"""
    worst_mean = worst_warp = 0.0
    for b in range(x.shape[0]):
        T, F = x[b].shape
        ref, m, y = sa.apply_clip(x[b], recs[b], fill)
        if not recs[b]["apply"]:
            np.testing.assert_array_equal(_bits(out[b]), _bits(x[b]), err_msg="%s: clip %d is not applied" % (what, b))
            continue
        if recs[b]["warp_center"] > 0:
            k, _ = sa.warp_taps(T, recs[b]["warp_center"], recs[b]["warp_shift"])
            bound = 4 * U * (np.abs(x[b][k]).astype(np.float64) + np.abs(x[b][k + 1]))
            err = np.abs(out[b] - y)
            assert (err[~m] <= bound[~m]).all(), "%s: clip %d warp error %g over its bound" % (what, b, (err - bound)[~m].max())
            if (~m).any():
                worst_warp = max(worst_warp, float((err[~m] / np.maximum(bound[~m], 1e-300)).max()))
            np.testing.assert_array_equal(_bits(out[b][[0, T - 1]][~m[[0, T - 1]]]), _bits(x[b][[0, T - 1]][~m[[0, T - 1]]]),
                                          err_msg="%s: clip %d: frames 0 and T - 1 map to themselves" % (what, b))
        else:
            np.testing.assert_array_equal(_bits(out[b][~m]), _bits(x[b][~m]), err_msg="%s: clip %d outside the masks" % (what, b))
        if fill == "zero":
            assert (_bits(out[b][m]) == 0).all(), "%s: clip %d: zero fill is exactly +0" % (what, b)
        else:
            tol = (T + 8) * U * float(np.abs(x[b]).max())
            err = np.abs(out[b] - ref)[m]
            if err.size:
                worst_mean = max(worst_mean, float(err.max()) / tol)
                assert err.max() <= tol, "%s: clip %d mean fill off by %g (%g)" % (what, b, err.max(), tol)
    return worst_mean, worst_warp


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_masks_without_warp_are_exact(torch, shape, B):
    from kws_amd.augment import FeatureMask
    T, F = shape
    rate = 0.5 if B >= 3 else 1.0
    base = _base_for(B, T, F, rate)
    x = _feats(B, T, F, seed=B)
    want = sa.np_draws(SEED ^ sa.MIX, STEP, base + np.arange(B), T, F, rate)
    on = want["apply"] == 1
    # the guard against an empty test, on the reference alone
    assert on.any() and 2 * (want["tw"][on].max(1) > 0).sum() >= on.sum() and 2 * (want["fw"][on].max(1) > 0).sum() >= on.sum()
    assert B < 3 or not on.all()
    figures = []
    for fill in ("zero", "mean"):
        fm = FeatureMask(rate=rate, fill=fill, seed=SEED)
        outs = []
        for in_place in (False, True):
            out, recs = _run(torch, fm, x, base=base, in_place=in_place)
            for name in sa.DTYPE.names:
                np.testing.assert_array_equal(recs[name], want[name], err_msg="plan_out." + name)
            for b in range(B):
                assert _same(recs[b], fm.draw(T, F, base + b, STEP))             # plan_out is kws_feature_mask_draw's plan
            got_mask = np.stack([_bits(out[b]) != _bits(x[b]) for b in range(B)])
            ref_mask = np.stack([sa.mask_of(want[b], T, F) & bool(want[b]["apply"]) for b in range(B)])
            assert not (got_mask & ~ref_mask).any(), "an entry outside every mask changed"
            figures.append(_check(out, x, recs, fill, "%s %s" % (fill, "in place" if in_place else "out of place"))[0])
            outs.append(out)
        np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]), err_msg="in place and out of place differ")
        if fill == "zero":
            changed = np.stack([_bits(outs[0][b]) != _bits(x[b]) for b in range(B)])
            assert (changed == (ref_mask & (x != 0))).all(), "the zeroed positions are the reference's masks"
    print("FIGURES mean fill %d x %d B=%d: worst error %.3g of the bound (T + 8) u max|x|" % (T, F, B, max(figures)))


def test_an_unaligned_base_takes_the_scalar_path_with_the_same_result(torch):
    """600 floats per clip allow 16-byte accesses only from an aligned base: a view that starts 4 bytes in gives the same bits"""
    from kws_amd.augment import FeatureMask
    B, T, F = 9, 30, 20
    x = _feats(B, T, F, seed=3)
    fm = FeatureMask(warp=2, rate=0.8, seed=SEED)
    want, _ = _run(torch, fm, x)
    buf = torch.zeros(B * T * F + 8, dtype=torch.float32, device="cuda")
    for off in (1, 2, 4):
        buf.zero_()
        view = buf[off:off + B * T * F].view(B, T, F)
        view.copy_(torch.from_numpy(x))
        assert (view.data_ptr() % 16 != 0) == (off != 4)
        out = fm(view, STEP, out=view)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
        assert float(buf[:off].abs().sum()) == 0 and float(buf[off + B * T * F:].abs().sum()) == 0


WARP_CASES = [(30, 20, 1), (30, 20, 3), (7, 13, 2)]


@pytest.mark.parametrize("T,F,W", WARP_CASES)
def test_warp_at_its_extremes(torch, T, F, W):
    from kws_amd.augment import FeatureMask
    plans = np.array([sa.record(c=c, d=d) for c in (W + 1, T - 2 - W) for d in (-W, 0, W)])
    B = len(plans)
    x = _feats(B, T, F, seed=W)
    fm = FeatureMask(time_masks=0, freq_masks=0, time_width=0, freq_width=0, seed=SEED)
    worst = 0.0
    for in_place in (False, True):
        out, recs = _run(torch, fm, x, in_place=in_place, plan=plans)
        assert _same(recs, plans)
        worst = max(worst, _check(out, x, recs, "mean", "warp W=%d" % W)[1])
        for b in range(B):
            np.testing.assert_array_equal(_bits(out[b][[0, T - 1]]), _bits(x[b][[0, T - 1]]))
            k, fr = sa.warp_taps(T, plans[b]["warp_center"], plans[b]["warp_shift"])
            if plans[b]["warp_shift"] == 0:                  # the identity, within the warp's own bound of the input
                assert (np.abs(out[b].astype(np.float64) - x[b]) <= 4 * U * (np.abs(x[b][k]).astype(np.float64) + np.abs(x[b][k + 1]))).all()
            else:
                assert np.abs(out[b] - x[b]).max() > 1.0     # and a shifted centre does move the frames
    print("FIGURES warp T=%d W=%d: worst error %.3g of the bound 4 u (|x[k]| + |x[k+1]|)" % (T, W, worst))


def _edge_plans(T, F, c, d):
    return np.array([
        sa.record(c=c, d=d, time=[(3, 0)], freq=[(5, 0)]),                                        # width 0: a no-op
        sa.record(c=c, d=d, time=[(0, T)]),                                                       # width T
        sa.record(c=c, d=d, freq=[(0, F)]),                                                       # width F
        sa.record(c=c, d=d, time=[(T - 2, 2)], freq=[(F - 3, 3)]),                                # ending exactly at T and at F
        sa.record(c=c, d=d, time=[(1, 3), (2, 3)]),                                               # two overlapping time masks
        sa.record(c=c, d=d, time=[(0, 1), (2, 1), (4, 2), (T - 1, 1)], freq=[(0, 2), (1, 2), (6, 1), (F - 1, 1)]),   # four of each
        sa.record(apply=0, c=c, d=d, time=[(0, T)], freq=[(0, F)]),                               # not applied: untouched
    ])


@pytest.mark.parametrize("fill", ["zero", "mean"])
@pytest.mark.parametrize("T,F,W", [(30, 20, 0), (30, 20, 3), (7, 13, 0), (7, 13, 2), (124, 40, 5)])
def test_edges_through_explicit_plans(torch, T, F, W, fill):
    from kws_amd.augment import FeatureMask
    plans = _edge_plans(T, F, W + 1 if W else 0, W)
    x = _feats(len(plans), T, F, seed=7)
    fm = FeatureMask(fill=fill, seed=SEED)
    for in_place in (False, True):
        out, recs = _run(torch, fm, x, in_place=in_place, plan=plans)
        assert _same(recs, plans)
        wm, ww = _check(out, x, recs, fill, "edges W=%d %s" % (W, fill))
        y0 = sa.warped(x[0], plans[0])
        if W == 0:
            np.testing.assert_array_equal(_bits(out[0]), _bits(x[0]))                             # width 0 without warp: nothing moves
        else:
            assert np.abs(out[0] - y0).max() <= 8 * U * 60.0
        if fill == "mean":                                                                        # the whole clip is its column means
            assert (out[1] == out[1][0][None, :]).all() and (out[2] == out[2][0][None, :]).all()
        else:
            assert not out[1].any() and not out[2].any()
    print("FIGURES edges %d x %d W=%d %s: mean %.3g of (T + 8) u max|x|, warp %.3g of 4 u (|x[k]| + |x[k+1]|)" % (T, F, W, fill, wm, ww))


def test_invalid_explicit_plans_are_reported(torch):
    from kws_amd import KwsError
    from kws_amd.augment import FeatureMask
    T, F = 30, 20
    x = torch.from_numpy(_feats(1, T, F)).cuda()
    keep = x.clone()
    fm = FeatureMask()
    for bad in (sa.record(apply=2), sa.record(time=[(28, 3)]), sa.record(time=[(-1, 2)]), sa.record(freq=[(0, 21)]), sa.record(freq=[(3, -1)]),
                sa.record(c=0, d=1), sa.record(c=29, d=0), sa.record(c=5, d=-5), sa.record(c=20, d=9)):
        with pytest.raises(KwsError) as e:
            fm(x, 0, out=x, plan=np.array([bad]))
        assert e.value.code == -1
    r = sa.record()
    r["n_time"] = 5
    with pytest.raises(KwsError):
        fm(x, 0, out=x, plan=np.array([r]))
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


@pytest.mark.parametrize("T,F", [(128, 40), (1, 5120)])
def test_the_largest_clip(torch, T, F):
    """kws_feature_mask_max_clip() floats per clip; one frame of 5120 coefficients needs the whole LDS budget of a block"""
    from kws_amd import KwsError
    from kws_amd import lib as l
    from kws_amd.augment import FeatureMask
    assert T * F == l.get_lib().kws_feature_mask_max_clip()
    B = 5
    x = _feats(B, T, F, seed=1)
    fm = FeatureMask(time_width=min(T, 4), warp=2 if T > 1 else 0, seed=SEED)
    out, recs = _run(torch, fm, x)
    want = sa.np_draws(SEED ^ sa.MIX, STEP, np.arange(B), T, F, 1.0, 2, min(T, 4), 2, 3, 2 if T > 1 else 0)
    assert _same(recs, want)
    _check(out, x, recs, "mean", "largest clip")
    with pytest.raises(KwsError) as e:
        fm(torch.zeros((1, T, F + 1), device="cuda"), 0)
    assert e.value.code == -2


def test_deterministic_keyed_by_step_and_shard_invariant(torch):
    from kws_amd.augment import FeatureMask
    T, F = 30, 20
    x = _feats(8, T, F, seed=5)
    fm = FeatureMask(warp=2, rate=0.7, seed=SEED)
    a, ra = _run(torch, fm, x, base=16)
    b, rb = _run(torch, fm, x, base=16)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert _same(ra, rb)
    c, rc = _run(torch, fm, x, base=16, step=STEP + 1)
    assert not _same(ra, rc) and not np.array_equal(_bits(a), _bits(c))
    whole, _ = _run(torch, fm, x, base=0)
    lo, _ = _run(torch, fm, x[:4], base=0)
    hi, _ = _run(torch, fm, x[4:], base=4)
    np.testing.assert_array_equal(_bits(whole), _bits(np.concatenate([lo, hi])))
    empty = fm(torch.zeros((0, T, F), device="cuda"), STEP)
    assert tuple(empty.shape) == (0, T, F)
