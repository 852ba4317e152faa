"""numpy restatement of the feature-mask stage (include/kws.h: kws_feature_mask_draw, kws_feature_mask), written from the definition
there: the draws field by field, the warp's source positions in float32 with the stated operations, everything else in float64."""
import numpy as np

from aug_ref import np_hash, np_uniform, np_unit

MIX = 0xE7037ED1A0B428DB          # kws_amd passes FeatureMask seed ^ MIX
FIELDS = 32
MAX_MASKS = 4
U = 2.0 ** -24

DTYPE = np.dtype([("apply", "<i4"), ("warp_center", "<i4"), ("warp_shift", "<i4"), ("n_time", "<i4"), ("n_freq", "<i4"),
                  ("t0", "<i4", (MAX_MASKS,)), ("tw", "<i4", (MAX_MASKS,)), ("f0", "<i4", (MAX_MASKS,)), ("fw", "<i4", (MAX_MASKS,))])


def np_draws(seed_m, step, positions, T, F, rate=1.0, n_time=2, time_width=4, n_freq=2, freq_width=3, warp=0):
    """the plans of the clips at the global positions `positions`, as DTYPE records (seed_m: the seed the kernel gets)"""
    pos = np.asarray(positions, np.uint64).reshape(-1)
    base = np.uint64(FIELDS) * pos

    def h(f):
        return np_hash(seed_m, step, base + np.uint64(f))

    out = np.zeros(pos.size, DTYPE)
    out["apply"] = np_unit(h(0)) < np.float32(rate)
    if warp > 0:
        out["warp_center"] = warp + 1 + np_uniform(h(1), T - 2 * warp - 2)
        out["warp_shift"] = np_uniform(h(2), 2 * warp + 1) - warp
    out["n_time"], out["n_freq"] = n_time, n_freq
    for i in range(n_time):
        w = np_uniform(h(3 + 2 * i), time_width + 1)
        out["tw"][:, i] = w
        out["t0"][:, i] = np_uniform(h(4 + 2 * i), T - w + 1)
    for j in range(n_freq):
        w = np_uniform(h(11 + 2 * j), freq_width + 1)
        out["fw"][:, j] = w
        out["f0"][:, j] = np_uniform(h(12 + 2 * j), F - w + 1)
    return out


def record(apply=1, c=0, d=0, time=(), freq=()):
    """one DTYPE record from (start, width) pairs"""
    r = np.zeros((), DTYPE)
    r["apply"], r["warp_center"], r["warp_shift"], r["n_time"], r["n_freq"] = apply, c, d, len(time), len(freq)
    for i, (s, w) in enumerate(time):
        r["t0"][i], r["tw"][i] = s, w
    for j, (s, w) in enumerate(freq):
        r["f0"][j], r["fw"][j] = s, w
    return r


def warp_positions(T, c, d):
    """float32 source position of every output frame, with exactly the definition's operations"""
    t = np.arange(T, dtype=np.int64)
    cd = int(c) + int(d)
    s = np.empty(T, np.float32)
    lo = t <= cd
    s[lo] = (t[lo] * int(c)).astype(np.float32) / np.float32(cd)
    s[~lo] = np.float32(c) + ((t[~lo] - cd) * (T - 1 - int(c))).astype(np.float32) / np.float32(T - 1 - cd)
    return s


def warp_taps(T, c, d):
    """-> (k, fr): the two taps k, k + 1 and the float32 weight of every output frame"""
    s = warp_positions(T, c, d)
    k = np.minimum(s.astype(np.int64), T - 2)
    return k, (s - k.astype(np.float32)).astype(np.float32)


def warped(x, rec):
    """float64 y of one clip x (T, F): interpolated from the float32 positions"""
    x = np.asarray(x, np.float64)
    if rec["warp_center"] <= 0:
        return x.copy()
    k, fr = warp_taps(x.shape[0], rec["warp_center"], rec["warp_shift"])
    fr = fr.astype(np.float64)[:, None]
    return (1.0 - fr) * x[k] + fr * x[k + 1]


def mask_of(rec, T, F):
    m = np.zeros((T, F), bool)
    for i in range(int(rec["n_time"])):
        m[rec["t0"][i]:rec["t0"][i] + rec["tw"][i], :] = True
    for j in range(int(rec["n_freq"])):
        m[:, rec["f0"][j]:rec["f0"][j] + rec["fw"][j]] = True
    return m


def apply_clip(x, rec, fill):
    """-> (out float64 (T, F), mask bool (T, F), y float64): one clip under its plan; fill 'zero' or 'mean'"""
    x = np.asarray(x, np.float64)
    T, F = x.shape
    if not rec["apply"]:
        return x.copy(), np.zeros((T, F), bool), x.copy()
    y = warped(x, rec)
    m = mask_of(rec, T, F)
    value = y.sum(0) / T if fill == "mean" else np.zeros(F)
    return np.where(m, value[None, :], y), m, y
