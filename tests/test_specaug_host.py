"""CPU tests of the feature-mask stage (include/kws.h: kws_feature_mask_draw, kws_feature_mask, kws_feature_mask_max_clip;
kws_amd.augment.FeatureMask; train.py's flags): the host draws against the numpy restatement of tests/specaug_ref.py, their bounds and
shares, the argument errors and the command line.  None of it needs a GPU."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import specaug_ref as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
SHAPES = {(30, 20): 3, (7, 13): 2, (124, 40): 5}            # (T, F): the widest warp the draw test uses there
POSITIONS = np.arange(4096)


def _draw_all(fm, T, F, positions, step):
    from kws_amd import lib as l
    L = l.get_lib()
    p = fm.params()
    rec = l.KwsFmaskClip()
    out = np.zeros(len(positions), sa.DTYPE)
    for i, pos in enumerate(positions):
        assert L.kws_feature_mask_draw(ctypes.byref(p), T, F, int(pos), step, ctypes.byref(rec)) == 0
        out[i] = np.frombuffer(bytes(rec), sa.DTYPE)[0]
    return out


def _fields_equal(a, b):
    for name in sa.DTYPE.names:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def test_record_and_params_layouts_match_the_header():
    from kws_amd import lib as l
    from kws_amd.augment import FMASK_DTYPE, FMASK_SEED_MIX, FILTER_SEED_MIX, REVERB_SEED_MIX, SPEED_SEED_MIX
    assert ctypes.sizeof(l.KwsFmaskClip) == sa.DTYPE.itemsize == FMASK_DTYPE.itemsize == 84 and FMASK_DTYPE == sa.DTYPE
    assert ctypes.sizeof(l.KwsFeatureMaskParams) == 40 and l.KwsFeatureMaskParams.seed.offset == 32
    assert FMASK_SEED_MIX == sa.MIX and FMASK_SEED_MIX % 2 == 1 and 2 ** 63 < FMASK_SEED_MIX < 2 ** 64
    assert len({FMASK_SEED_MIX, FILTER_SEED_MIX, REVERB_SEED_MIX, SPEED_SEED_MIX}) == 4
    with open(os.path.join(ROOT, "include", "kws.h")) as f:
        h = f.read()
    for word in ("kws_feature_mask_params", "kws_fmask_clip", "kws_feature_mask_draw", "kws_feature_mask_max_clip", "0xE7037ED1A0B428DB",
                 "KWS_FMASK_ZERO", "KWS_FMASK_MEAN", "#define KWS_FMASK_MAX 4"):
        assert word in h, word


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_host_draws_equal_the_numpy_draws_field_by_field(shape):
    from kws_amd.augment import FeatureMask
    T, F = shape
    W = SHAPES[shape]
    # the last positions wrap 32 p past 2^32, as the kernel's 32-bit index does
    positions = np.concatenate([POSITIONS, 2 ** 27 - 2 + np.arange(4)])
    for seed in (0, 0x123456789ABCDEF):
        fm = FeatureMask(time_masks=4, time_width=min(T, 5), freq_masks=3, freq_width=min(F, 6), warp=W, rate=0.5, seed=seed)
        for step in (0, 1, 977):
            got = _draw_all(fm, T, F, positions, step)
            want = sa.np_draws(seed ^ sa.MIX, step, positions, T, F, 0.5, 4, min(T, 5), 3, min(F, 6), W)
            _fields_equal(got, want)


def test_feature_mask_draw_method_and_shard_equivalence():
    """position_base + b draws the same whatever the split: the draw depends on the global position alone"""
    from kws_amd.augment import FeatureMask
    fm = FeatureMask(warp=2, rate=0.7, seed=9)
    whole = _draw_all(fm, 30, 20, np.arange(64), 5)
    for base, n in ((0, 24), (24, 8), (32, 32)):
        part = np.array([fm.draw(30, 20, base + b, 5) for b in range(n)])
        _fields_equal(part, whole[base:base + n])
    assert not np.array_equal(_draw_all(fm, 30, 20, np.arange(64), 6), whole)                    # another step draws afresh
    assert not np.array_equal(_draw_all(FeatureMask(warp=2, rate=0.7, seed=10), 30, 20, np.arange(64), 5), whole)


def test_applied_share_is_the_rate():
    """4096 Bernoulli(0.5) draws: 0.5 +- 4 sigma = 0.5 +- 4 sqrt(0.25 / 4096) = 0.5 +- 0.03125 (the issue rounds to 0.032); the seed is
    fixed, so this is a property of the hash"""
    from kws_amd.augment import FeatureMask
    got = _draw_all(FeatureMask(rate=0.5, seed=1), 30, 20, POSITIONS, 3)
    share = got["apply"].mean()
    print("FIGURES applied share at rate 0.5 over 4096 positions: %.4f (0.5 +- 0.032)" % share)
    assert abs(share - 0.5) <= 0.032
    assert _draw_all(FeatureMask(rate=0.0, seed=1), 30, 20, POSITIONS[:256], 3)["apply"].sum() == 0
    assert _draw_all(FeatureMask(rate=1.0, seed=1), 30, 20, POSITIONS[:256], 3)["apply"].sum() == 256


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_draws_stay_inside_the_clip_and_reach_both_ends(shape):
    from kws_amd.augment import FeatureMask
    T, F = shape
    W = SHAPES[shape]
    tw, fw = min(T, 4), min(F, 3)
    got = _draw_all(FeatureMask(time_masks=4, time_width=tw, freq_masks=4, freq_width=fw, warp=W, seed=2), T, F, POSITIONS, 1)
    assert (got["t0"] >= 0).all() and (got["t0"] + got["tw"] <= T).all()
    assert (got["f0"] >= 0).all() and (got["f0"] + got["fw"] <= F).all()
    assert got["tw"].min() == 0 and got["tw"].max() == tw and got["fw"].min() == 0 and got["fw"].max() == fw
    assert (got["t0"] + got["tw"]).max() == T and (got["f0"] + got["fw"]).max() == F and got["t0"].min() == 0 and got["f0"].min() == 0
    c, cd = got["warp_center"], got["warp_center"] + got["warp_shift"]
    assert c.min() == W + 1 and c.max() == T - 2 - W
    assert got["warp_shift"].min() == -W and got["warp_shift"].max() == W
    assert cd.min() >= 1 and cd.max() <= T - 2
    # full-width masks are allowed by the parameters
    full = _draw_all(FeatureMask(time_masks=1, time_width=T, freq_masks=1, freq_width=F, seed=2), T, F, POSITIONS, 1)
    assert full["tw"].max() == T and full["fw"].max() == F and (full["t0"][:, 0] + full["tw"][:, 0] <= T).all()


def _params(**kw):
    from kws_amd import lib as l
    p = l.KwsFeatureMaskParams()
    p.rate, p.n_time, p.max_time_width, p.n_freq, p.max_freq_width, p.max_warp, p.fill, p.seed = 1.0, 2, 4, 2, 3, 0, 1, 5
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD = [(dict(rate=-0.1), b"rate"), (dict(rate=1.5), b"rate"), (dict(rate=float("nan")), b"rate"),
       (dict(n_time=-1), b"time masks"), (dict(n_time=5), b"time masks"), (dict(n_freq=-1), b"frequency masks"),
       (dict(n_freq=5), b"frequency masks"), (dict(max_time_width=-1), b"max_time_width"), (dict(max_time_width=31), b"max_time_width"),
       (dict(max_freq_width=-1), b"max_freq_width"), (dict(max_freq_width=21), b"max_freq_width"), (dict(max_warp=14), b"time warp"),
       (dict(max_warp=-1), b"max_warp"), (dict(fill=2), b"fill")]


@pytest.mark.parametrize("bad,word", BAD)
def test_invalid_parameters_are_reported_host_side(bad, word):
    from kws_amd import lib as l
    L = l.get_lib()
    rec = l.KwsFmaskClip()
    p = _params(**bad)
    for rc in (L.kws_feature_mask_draw(ctypes.byref(p), 30, 20, 0, 0, ctypes.byref(rec)),
               L.kws_feature_mask(ctypes.byref(p), None, None, 0, 30, 20, 0, 0, None, None, None)):
        assert rc == l.ERR_INVALID and word in L.kws_last_error(), (rc, L.kws_last_error())


def test_limits_need_no_device():
    from kws_amd import lib as l
    L = l.get_lib()
    rec = l.KwsFmaskClip()
    ok = _params()
    assert L.kws_feature_mask_draw(ctypes.byref(_params(max_warp=13)), 29, 20, 0, 0, ctypes.byref(rec)) == 0       # T = 2 W + 3
    assert L.kws_feature_mask_draw(ctypes.byref(_params(max_warp=13)), 28, 20, 0, 0, ctypes.byref(rec)) == l.ERR_INVALID
    assert L.kws_feature_mask_draw(ctypes.byref(_params(max_time_width=30, max_freq_width=20)), 30, 20, 0, 0, ctypes.byref(rec)) == 0
    assert L.kws_feature_mask_draw(None, 30, 20, 0, 0, ctypes.byref(rec)) == l.ERR_INVALID
    assert L.kws_feature_mask_draw(ctypes.byref(ok), 30, 20, 0, 0, None) == l.ERR_INVALID
    assert L.kws_feature_mask_draw(ctypes.byref(ok), 30, 20, -1, 0, ctypes.byref(rec)) == l.ERR_INVALID
    assert L.kws_feature_mask_draw(ctypes.byref(ok), 0, 20, 0, 0, ctypes.byref(rec)) == l.ERR_INVALID
    cap = L.kws_feature_mask_max_clip()
    assert cap >= 124 * 40
    assert L.kws_feature_mask(ctypes.byref(ok), None, None, 0, cap // 40, 40, 0, 0, None, None, None) == 0        # B == 0: no launch
    rc = L.kws_feature_mask(ctypes.byref(ok), None, None, 0, cap // 40 + 1, 40, 0, 0, None, None, None)
    assert rc == l.ERR_UNSUPPORTED and b"larger than" in L.kws_last_error()
    assert L.kws_feature_mask(ctypes.byref(ok), None, None, -1, 30, 20, 0, 0, None, None, None) == l.ERR_INVALID
    assert L.kws_feature_mask(ctypes.byref(ok), None, None, 0, 30, 20, -1, 0, None, None, None) == l.ERR_INVALID
    assert L.kws_feature_mask(ctypes.byref(ok), None, None, 1, 30, 20, 0, 0, None, None, None) == l.ERR_INVALID and \
        b"null" in L.kws_last_error()


def test_feature_mask_constructor_checks_its_arguments():
    from kws_amd.augment import FeatureMask
    fm = FeatureMask()
    assert (fm.time_masks, fm.time_width, fm.freq_masks, fm.freq_width, fm.warp, fm.rate, fm.fill, fm.seed) == (2, 4, 2, 3, 0, 1.0, "mean", 0)
    p = FeatureMask(time_masks=1, time_width=7, freq_masks=3, freq_width=2, warp=4, rate=0.25, fill="zero", seed=11).params()
    assert (p.rate, p.n_time, p.max_time_width, p.n_freq, p.max_freq_width, p.max_warp, p.fill, p.seed) == \
        (0.25, 1, 7, 3, 2, 4, 0, 11 ^ sa.MIX)
    for bad in (dict(time_masks=5), dict(freq_masks=-1), dict(time_width=-1), dict(freq_width=1.5), dict(warp=-2), dict(rate=1.1),
                dict(fill="median")):
        with pytest.raises(ValueError):
            FeatureMask(**bad)
    from kws_amd import KwsError
    with pytest.raises(KwsError) as e:
        FeatureMask(time_width=31).draw(30, 20, 0, 0)
    assert e.value.code == -1 and "max_time_width" in str(e.value)


def _train_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_train_py_mask_flags(capsys):
    from kws_amd.augment import FeatureMask
    train = _train_module("kws_train_main_fmask")
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--time_mask", "--freq_mask", "--time_warp", "--mask_rate", "--mask_fill"):
        assert flag in text
    base = ["--train_data_path", "d", "--classes_path", "c"]
    for extra in ([], ["--raw_audio"]):
        a = train.parse_args(base + extra)
        assert (a.time_mask, a.freq_mask, a.time_warp, a.mask_rate, a.mask_fill) == (None, None, None, None, None)
        assert train.mask_options(a) == {}                  # no flag: no FeatureMask object
        kw = train.mask_options(train.parse_args(base + extra + ["--time_mask", "2,4", "--freq_mask", "1,3", "--time_warp", "2",
                                                                 "--mask_rate", "0.5", "--mask_fill", "zero"]))
        assert kw == dict(time_masks=2, time_width=4, freq_masks=1, freq_width=3, warp=2, rate=0.5, fill="zero")
        fm = FeatureMask(**kw)
        assert (fm.time_masks, fm.time_width, fm.freq_masks, fm.freq_width, fm.warp, fm.rate, fm.fill) == (2, 4, 1, 3, 2, 0.5, "zero")
    kw = train.mask_options(train.parse_args(base + ["--freq_mask", "2,3"]))
    assert kw == dict(time_masks=0, time_width=0, freq_masks=2, freq_width=3, warp=0, rate=1.0, fill="mean")
    assert train.mask_options(train.parse_args(base + ["--time_warp", "3"]))["warp"] == 3
    for bad in (["--time_mask", "2"], ["--time_mask", "a,b"], ["--time_mask", "5,2"], ["--freq_mask", "2,-1"], ["--time_warp", "-1"],
                ["--time_mask", "2,4", "--mask_rate", "1.5"], ["--mask_rate", "0.5"], ["--mask_fill", "zero"]):
        with pytest.raises(SystemExit):
            train.mask_options(train.parse_args(base + bad))
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--time_mask", "2,4", "--mask_fill", "median"])
