"""Case table of the tempo/pitch stage at its chunk, plan, tile and long-clip edges (tests/test_pitch_edges_host.py,
tests/test_pitch_edges_gpu.py): pitch_stft_kernel and pitch_synth_kernel (csrc/kws_pitch.hip).

What the kernels are made of, restated here.  N in {256, 512, 1024}, hop H = N / 4, G = 2048 / N frames per block, so a chunk of the
synthesis completes G H = 512 samples at every N and carries 3 H.  Per clip the device plans (clip_plan) what max_samples outputs need:
`need` stretched samples, Jn of Jtot output frames, Mn of M analysis frames, each capped by what a slot of the workspace holds
(need_cap, mn_cap: Slots of the call's own ranges).  plan(), slots() and call_ranges() restate that arithmetic in float64 with r and
rho from pitch_ref; labels() derives from it where a clip sits against every such edge.  perturb_planned() is pitch_ref's vocoder cut
down to the plan, so the host can show that the plan is sufficient without a device.

Groups (one Call = one kws_pitch_apply; every clip carries the labels it is there for in `claims`):
    A  lengths   N = 512 / 1024 at source lengths on both sides of H, N and 2 N, explicit tempos, shifts alone and with a tempo
    B  chunks    tempo only, need = max_samples one below, at and one above k 512 - N / 2; sources that end inside the output with
                 Jn == Jtot at every residue mod G
    C  ratios    tempo 1, shifts +0, -0 and 1e-7 (r == 1.0f: vocoded, not resampled), the two smallest shifts with r != 1, the float32
                 neighbours of 0.5, 1 and 2, rho = 4, 0.25, 2, 0.5, 1.25
    D  caps      a clip at need_cap, a clip at mn_cap, a short one; and a call no clip of which has the call's rho_max
    E  tiles     24 drawn clips through a repeated unordered index, valid_len and a position base
    F  batches   96 (source, pair) combinations at max_samples 8, repeated past 32768 clips
    G  frames    kws_pitch_stft's `frames` around G, 2 G, 3 G and 4 G (no Call: the analysis alone)
    H  long      max_samples = stride = 16000, 64000 samples of a steady tone, and one clip at max_samples = 1 << 20
    I  table     the resampler's table against the vocoder's LDS at N = 512 and 1024

Host only: numpy, the float64 restatements and test_pitch_gpu.py's source generator."""
import collections
import functools
import math
import zlib

import numpy as np

import pitch_ref as pf
import speed_mix_cases as sm
import speed_ref as sr
from test_pitch_gpu import LENGTHS, RATES, SEMITONES, _source

F32 = np.float32
NAN = float("nan")
CHUNK = 512                                        # G H at every N: the samples a chunk of the synthesis completes
KMAX_SAMPLES = 1 << 20                             # csrc/kws_pitch.hip: kMaxSamples
KMAX_Z = 32                                        # csrc/kws_pitch.hip: kMaxZ
TILE_CEILING = 32768                               # kws_pitch_apply: tile = fit < 32768 ? fit : 32768; kws_pitch_stft: b0 += 32768
PAD = 7                                            # out_stride = max_samples + PAD, prefilled with 9.0
NO_CAP = 1 << 30


def geometry(N):
    """-> (H, G)"""
    return N // 4, 2048 // N


# ---- clip_plan, Slots and the call's ranges, restated ------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "vocoded r rho M Jtot Lst lo need Jn Mn")
Slots = collections.namedtuple("Slots", "need_max jn_max mn_max spec_stride st_stride clip_bytes")


def plan(Ls, tempo, semis, max_samples, N, Z, need_cap=NO_CAP, mn_cap=NO_CAP):
    """csrc/kws_pitch.hip clip_plan: what max_samples outputs of a clip of Ls samples need of the vocoder"""
    H = N // 4
    r, rho = float(pf.ratio(semis)), pf.rho(tempo, semis)
    M = 1 + Ls // H
    if float(F32(tempo)) == 0.0 and np.isnan(semis):
        return Plan(False, r, rho, M, 0, Ls, min(Ls, max_samples), 0, 0, 0)
    Jtot = int(math.ceil(M / rho))
    Lst = math.floor(Ls / rho + 0.5)
    lo = math.ceil(Lst / r) if r != 1.0 else Lst
    lo = int(min(lo, max_samples))
    if lo == 0:
        return Plan(True, r, rho, M, Jtot, int(Lst), 0, 0, 0, 0)
    need = float(lo)
    if r != 1.0:
        s = 1.0 / r if r > 1.0 else 1.0
        need = min(math.floor((lo - 1.0) * r) + 2.0 + math.ceil(Z / s), Lst)
    need = int(min(need, need_cap))
    Jn = min((need + N // 2 + H - 1) // H, Jtot)
    Mn = int(min(math.floor((Jn - 1) * rho) + 2.0, M, mn_cap))
    return Plan(True, r, rho, M, Jtot, int(Lst), lo, need, Jn, Mn)


def slots(N, max_samples, rho_max=4.0, r_max=2.0, Z=KMAX_Z):
    """csrc/kws_pitch.hip Slots: what a clip can need when no clip's rho exceeds rho_max and no clip's r exceeds r_max"""
    H = N // 4
    need_max = int(math.floor((max_samples - 1) * r_max)) + 2 + int(math.ceil(Z * (r_max if r_max > 1.0 else 1.0)))
    jn_max = (need_max + N // 2 + H - 1) // H
    mn_max = int(math.floor((jn_max - 1) * rho_max)) + 2
    spec = (mn_max * (N // 2 + 1) + 15) // 16 * 16
    st = (need_max + 31) // 32 * 32
    return Slots(need_max, jn_max, mn_max, spec, st, spec * 8 + st * 4)


def call_ranges(tempo, semis):
    """kws_pitch_apply with explicit tempos and shifts: -> (tempo_max, r_min, r_max), the ends its tiles are sized for"""
    tempo_max, n_lo, n_hi = F32(1.0), F32(0.0), F32(0.0)
    for t in np.asarray(tempo, F32):
        tempo_max = t if t > tempo_max else tempo_max
    for n in np.asarray(semis, F32):
        if not np.isnan(n):
            n_lo, n_hi = (n if n < n_lo else n_lo), (n if n > n_hi else n_hi)
    return float(tempo_max), float(F32(2.0 ** (float(n_lo) / 12.0))), float(F32(2.0 ** (float(n_hi) / 12.0)))


# ---- the table's records -----------------------------------------------------------------------------------------------------------------
# one clip: its source length, tempo (0: not stretched), shift (NaN: not pitched), whether it is _source's badly conditioned row, and the
# label values it is in the table for
Clip = collections.namedtuple("Clip", "ls tempo semis hard claims")
# one kws_pitch_apply: table = a key of speed_mix_cases.TABLES, or None for a call without a resampler (Z = 0)
Call = collections.namedtuple("Call", "group name N max_samples stride table clips")


def _clip(ls, tempo=0.0, semis=NAN, hard=False, **claims):
    return Clip(int(ls), F32(tempo), F32(semis), bool(hard), claims)


def call_z(call):
    return 0 if call.table is None else sm.TABLES[call.table][0]


def call_slots(call):
    """the Slots kws_pitch_apply sizes this call's tiles with: need_cap = need_max, mn_cap = mn_max"""
    tempo_max, r_min, r_max = call_ranges([c.tempo for c in call.clips], [c.semis for c in call.clips])
    return slots(call.N, call.max_samples, tempo_max / r_min, r_max, call_z(call))


def clip_plan(call, clip, sl=None):
    sl = sl or call_slots(call)
    return plan(clip.ls, clip.tempo, clip.semis, call.max_samples, call.N, call_z(call), sl.need_max, sl.mn_max)


def advances(p):
    """the set of floor(j rho) - floor((j - 1) rho) over the output frames the device makes"""
    fl = [math.floor(j * p.rho) for j in range(p.Jn)]
    return frozenset(b - a for a, b in zip(fl, fl[1:]))


def labels(call, clip, sl=None):
    """where the clip sits against the kernels' edges"""
    sl = sl or call_slots(call)
    p = clip_plan(call, clip, sl)
    _, G = geometry(call.N)
    span = p.need + call.N // 2 if p.lo > 0 else 0
    adv = advances(p)
    return dict(vocoded=p.vocoded, chunks=(span + CHUNK - 1) // CHUNK, chunk_mod=span % CHUNK, jn_mod_g=p.Jn % G, jn_lt_jtot=p.Jn < p.Jtot,
                mn_lt_m=p.Mn < p.M, at_need_cap=p.lo > 0 and p.need == sl.need_max, at_mn_cap=p.lo > 0 and p.Mn == sl.mn_max,
                adv=adv, adv_class=frozenset(min(a, 2) for a in adv), resampled=p.vocoded and p.r != 1.0, lo=p.lo)


def layout(call):
    """-> (lens (rows,) int32, index (B,) int32): one loud row of _source per distinct length, then its badly conditioned row (the last
    but one, as _source has it) and a spare"""
    loud = sorted({c.ls for c in call.clips if not c.hard})
    hard = sorted({c.ls for c in call.clips if c.hard})
    assert len(hard) <= 1 and call.stride >= 500 and max(c.ls for c in call.clips) <= call.stride
    lens = np.array(loud + (hard or [0]) + [0], np.int32)
    index = np.array([len(loud) if c.hard else loud.index(c.ls) for c in call.clips], np.int32)
    return lens, index


def source(call, i16):
    """-> (x (rows, stride), lens, index, tempo, semis) of the call"""
    lens, index = layout(call)
    x = _source(i16, rows=len(lens), stride=call.stride, seed=zlib.crc32(call.name.encode()) & 0xFFFF)
    return x, lens, index, np.array([c.tempo for c in call.clips], F32), np.array([c.semis for c in call.clips], F32)


# ---- the vocoder cut down to the plan ----------------------------------------------------------------------------------------------------
def vocoder_planned(D, rate, N, need, Jn, Mn):
    """pitch_ref.vocoder reading nothing from the frames Mn on and making the frames j < Jn only -> the first `need` stretched samples"""
    D = np.array(D, np.complex128)
    D[Mn:] = 0.0
    K, H = D.shape[1], N // 4
    Dp = np.vstack([D, np.zeros((2 + max(0, int(math.floor(Jn * rate)) + 2 - len(D)), K), np.complex128)])
    k = np.arange(K)
    w = pf.window(N)
    out, wss = (np.zeros(max((Jn - 1) * H + N, N // 2 + need)) for _ in range(2))
    phi = pf._ang(Dp[0])
    for j in range(Jn):
        t = j * rate
        m0 = int(math.floor(t))
        al = t - m0
        d0, d1 = Dp[m0], Dp[m0 + 1]
        mag = (1.0 - al) * np.abs(d0) + al * np.abs(d1)
        out[j * H:j * H + N] += w * np.fft.irfft(mag * pf._I_POW[(j * k) % 4] * np.exp(1j * phi), N)
        wss[j * H:j * H + N] += w * w
        dl = pf._ang(d1) - pf._ang(d0) - (np.pi / 2.0) * k
        phi = phi + (dl - 2.0 * np.pi * np.rint(dl / (2.0 * np.pi)))
    nz = wss > 1e-8
    out[nz] /= wss[nz]
    return out[N // 2:N // 2 + need]


def perturb_planned(D, p, N, tab, Jn=None, Mn=None):
    """the clip's lo outputs from the planned part of the vocoder alone: the resampler sees `need` stretched samples, as on the device"""
    h, Z, P = tab
    y = vocoder_planned(D, p.rho, N, p.need, p.Jn if Jn is None else Jn, p.Mn if Mn is None else Mn)
    return y[:p.lo] if p.r == 1.0 else sr.resample(y, p.r, p.lo, h, Z, P)[0]


# ---- shifts next to r = 1 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smallest_shift(sign):
    """the float32 shift of smallest magnitude, of the given sign, whose ratio() is not 1 (bisection over the float32 bit patterns)"""
    lo, hi = 0, int(F32(1.0).view(np.int32))                 # ratio(lo) == 1, ratio(hi) != 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pf.ratio(F32(sign) * np.int32(mid).view(F32)) != 1:
            hi = mid
        else:
            lo = mid
    return F32(sign) * np.int32(hi).view(F32)


# ---- the groups --------------------------------------------------------------------------------------------------------------------------
MS, STRIDE = 1024, 1100                            # test_pitch_gpu.py's geometry: its _both applies as it stands
LEN_A = {512: (0, 1, 127, 128, 129, 511, 512, 513, 1100), 1024: (0, 1, 255, 256, 257, 1023, 1024, 1025, 1100)}
TEMPO_PATTERN = (0.8, 1.25, 2.0, 0.5)              # test_pitch_gpu.py's test 2
CHUNK_MS = {256: (383, 384, 385, 895, 896, 897), 512: (255, 256, 257, 767, 768, 769), 1024: (1, 511, 512, 513, 1023, 1024, 1025)}
CHUNK_TEMPOS = (0.8, 1.25)
LONG_MS = 16000
TONE_MS = 64000
LONG_PAIRS = ((0.5, NAN), (2.0, NAN), (1.0, NAN), (0.0, 0.0), (0.5, 12.0), (2.0, -12.0), (0.8, 4.0))
LDS_TABLES = ((512, "z4p32"), (1024, "z4p32"), (1024, "default"))
# E: 9 rows, two of them with a valid_len outside [0, stride]
TILE_LENS = (0, -5, 63, STRIDE + 100, 65, 255, 256, 1000, 777)
TILE_INDEX = (8, 7, 7, 0, 5, 2, 8, 1, 6, 3, 4, 7, 3, 3, 0, 6, 8, 1, 5, 2, 4, 4, 7, 6)
TILE_SEED, TILE_STEP, TILE_BASE = 37, 3, 1000
TILE_DRAW = dict(tempo_rate=0.8, tempo=(0.5, 2.0), pitch_rate=0.8, pitch=(-12.0, 12.0))
TILE_WORKSPACES = (1, 5, 23)
# F: 16 source rows of 64 samples, 6 (tempo, shift) pairs, 96 combinations: clip b is row (b // 6) % 16 under pair b % 6
BATCH_MS, BATCH_STRIDE = 8, 64
BATCH_LENS = (64, 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 63, 64, 64)
BATCH_PAIRS = ((0.0, NAN), (0.5, NAN), (2.0, NAN), (0.0, 12.0), (2.0, -12.0), (0.8, 4.0))
BATCH_SIZES = (TILE_CEILING + 1, 2 * TILE_CEILING)


def frame_counts(N):
    """G: kws_pitch_stft's `frames`; 3 G + 1 and 4 G + 1 give a block a second group of frames (frame_blocks: two groups a block)"""
    _, G = geometry(N)
    return sorted({1, G - 1, G, G + 1, 2 * G, 2 * G + 1, 3 * G + 1, 4 * G + 1})


def frame_clips(N):
    """G: -> (stride, source lengths) with M = 1, G - 1, G, G + 1, 2 G + 1 and 3 G + 2 frames"""
    H, G = geometry(N)
    ms_ = sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1, 3 * G + 2})
    return (3 * G + 2) * H - 1, [0 if m == 1 else (m - 1) * H + (m % 3) * (H // 3) for m in ms_]


def frame_blocks(frames, N):
    """csrc/kws_pitch.hip frame_blocks"""
    _, G = geometry(N)
    groups = (frames + G - 1) // G
    return (groups + 1) // 2 if groups > 1 else 1


def _group_a():
    out = []
    for N in (512, 1024):
        for rate in RATES:
            out.append(Call("A", "A tempo %g N %d" % (rate, N), N, MS, STRIDE, None,
                            [_clip(ls, rate) for ls in LEN_A[N]] + [_clip(STRIDE, rate, hard=True)]))
        for n in SEMITONES:
            clips = [_clip(ls, 0.0, n, resampled=True) for ls in LEN_A[N]]
            clips += [_clip(ls, TEMPO_PATTERN[i % 4], n, resampled=True) for i, ls in enumerate(LEN_A[N])]
            out.append(Call("A", "A pitch %+g N %d" % (n, N), N, MS, STRIDE, "default", clips + [_clip(STRIDE, 0.0, n, hard=True)]))
    return out


def _residue_clips(N):
    """sources that end inside the output (Lst < max_samples) with Jn == Jtot at every residue mod G, the longest such source each"""
    _, G = geometry(N)
    out = []
    for res in range(G):
        tempo = CHUNK_TEMPOS[res % 2]
        for ls in range(STRIDE, 0, -1):
            p = plan(ls, tempo, NAN, MS, N, 0)
            if p.Jn == p.Jtot and p.Jn % G == res and p.lo == p.Lst < MS:
                out.append(_clip(ls, tempo, jn_mod_g=res, jn_lt_jtot=False))
                break
        else:
            raise AssertionError((N, res))
    return out


def _group_b():
    out = []
    for N in pf.N_FFTS:
        for ms in CHUNK_MS[N]:
            ls = 2 * ms + N                                  # Lst >= max_samples at both tempos
            out.append(Call("B", "B chunk N %d ms %d" % (N, ms), N, ms, max(ls, 600), None,
                            [_clip(ls, t, chunk_mod=(ms + N // 2) % CHUNK, chunks=(ms + N // 2 + CHUNK - 1) // CHUNK, lo=ms) for t in CHUNK_TEMPOS]))
        out.append(Call("B", "B residues N %d" % N, N, MS, STRIDE, None, _residue_clips(N)))
    return out


def ratio_pairs():
    """C: (tempo, shift, claims)"""
    up = lambda a, b: np.nextafter(F32(a), F32(b))
    same = dict(resampled=False, adv=frozenset([1]))
    return [(1.0, NAN, same), (0.0, 0.0, same), (0.0, -0.0, same), (0.0, 1e-7, same),
            (0.0, smallest_shift(1), dict(resampled=True)), (0.0, smallest_shift(-1), dict(resampled=True)),
            (up(0.5, 1), NAN, dict(adv_class=frozenset([0, 1]))), (up(1, 0), NAN, dict(adv_class=frozenset([0, 1]))),
            (up(1, 2), NAN, dict(adv=frozenset([1]))), (up(2, 0), NAN, dict(adv_class=frozenset([1, 2]))),
            (2.0, -12.0, dict(adv=frozenset([4]), resampled=True)), (0.5, 12.0, dict(adv=frozenset([0, 1]), resampled=True)),
            (2.0, NAN, dict(adv=frozenset([2]))), (0.5, NAN, dict(adv=frozenset([0, 1]))), (1.25, NAN, dict(mixed=True))]


def _group_c():
    out = []
    for N in pf.N_FFTS:
        clips = []
        for t, n, claims in ratio_pairs():
            if claims.pop("mixed", False) and N < 1024:          # 1100 samples are 4 output frames at N = 1024: floor(1.25 j) = 0, 1, 2, 3
                claims = dict(adv=frozenset([1, 2]))
            clips += [_clip(STRIDE, t, n, **claims), _clip(STRIDE, t, n, hard=True, **claims)]
        out.append(Call("C", "C ratios N %d" % N, N, MS, STRIDE, "default", clips))
    return out


CAP_SHIFT, CAP_TEMPO = 0.25, 1.25                   # D: shifts of +-0.25 semitones keep need_max and the mn_cap clip's need in one hop


@functools.lru_cache(maxsize=None)
def _cap_call(N):
    """the smallest max_samples from 1000 on at which (tempo 0, +0.25) meets need_cap and (1.25, -0.25) meets mn_cap, a short clip beside
    them: the first has the call's r_max, the second its rho_max, and their `need` must fall into the same hop for Mn to reach mn_max"""
    for ms in range(1000, 1400):
        stride = 2 * ms
        call = Call("D", "D caps N %d" % N, N, ms, stride, "default",
                    [_clip(stride, 0.0, CAP_SHIFT, at_need_cap=True), _clip(stride, CAP_TEMPO, -CAP_SHIFT, at_mn_cap=True),
                     _clip(100, 0.8, NAN, at_need_cap=False, at_mn_cap=False)])
        if all(all(labels(call, c)[k] == v for k, v in c.claims.items()) for c in call.clips):
            return call
    raise AssertionError(N)


def _group_d():
    out = [_cap_call(N) for N in pf.N_FFTS]
    for N in pf.N_FFTS:                                      # tempo_max from the first clip, r_min from the second
        out.append(Call("D", "D split ranges N %d" % N, N, MS, STRIDE, "default",
                        [_clip(STRIDE, 2.0, NAN), _clip(STRIDE, 0.0, -12.0), _clip(STRIDE, 0.8, 4.0), _clip(STRIDE, 0.8, 4.0, hard=True)]))
    return out


WIDEST = ((2.0, -12.0), (0.5, 12.0))               # D: two clips more give the call the widest ranges there are


def tile_values():
    """E: the draws of the 24 clips as explicit values"""
    on, t, pit, n = pf.np_draws(TILE_SEED, TILE_STEP, TILE_BASE + np.arange(len(TILE_INDEX)), **TILE_DRAW)
    return np.where(on, t, F32(0)).astype(F32), np.where(pit, n, F32(NAN)).astype(F32)


def tile_lens():
    """E: the valid lengths as the device reads them (csrc/kws_wave_stage.h clip_src)"""
    return np.clip(np.array(TILE_LENS, np.int64), 0, STRIDE).astype(np.int32)


def _group_e():
    tempo, semis = tile_values()
    lens = tile_lens()
    return [Call("E", "E tiles N %d" % N, N, MS, STRIDE, "default",
                 [_clip(lens[r], tempo[b], semis[b], hard=(r == len(TILE_LENS) - 2)) for b, r in enumerate(TILE_INDEX)]) for N in (256, 1024)]


def batch_clip(b):
    """F: -> (row, tempo, shift) of clip b of any batch"""
    t, n = BATCH_PAIRS[b % 6]
    return (b // 6) % 16, t, n


def _group_f():
    clips = []
    for b in range(96):
        row, t, n = batch_clip(b)
        clips.append(_clip(BATCH_LENS[row], t, n))
    return [Call("F", "F batch", 256, BATCH_MS, BATCH_STRIDE, "default", clips)]


def _group_h():
    out = []
    for N in pf.N_FFTS:
        for t, n in LONG_PAIRS:
            out.append(Call("H", "H long N %d tempo %g shift %g" % (N, t, n), N, LONG_MS, LONG_MS, None if np.isnan(n) else "default",
                            [_clip(LONG_MS, t, n), _clip(9000, t, n), _clip(LONG_MS, t, n, hard=True)]))
    # 4 s of the badly conditioned row's steady 700 Hz tone at rho = 1: a phase advance that is wrong by the same amount in every frame
    # grows by the frame, and 1001 frames show what 251 do not (1.10 bounds before the advance was mended)
    out.append(Call("H", "H tone N 256 ms %d" % TONE_MS, 256, TONE_MS, TONE_MS, None,
                    [_clip(TONE_MS, 1.0), _clip(9000, 1.0), _clip(TONE_MS, 1.0, hard=True)]))
    return out


def largest_call(ms=KMAX_SAMPLES):
    """H: one clip at the largest max_samples the stage accepts, tempo 2"""
    return Call("H", "H largest %d" % ms, 256, ms, 2 * ms, None, [_clip(2 * ms, 2.0, NAN, lo=ms)])


def _group_i():
    out = []
    for N, name in LDS_TABLES:
        clips = [_clip(ls, 0.0, n, resampled=True) for n in (-12.0, -4.0, 4.0, 12.0) for ls in LENGTHS]
        out.append(Call("I", "I table %s N %d" % (name, N), N, MS, STRIDE, name, clips + [_clip(STRIDE, 0.0, 4.0, hard=True)]))
    return out


@functools.lru_cache(maxsize=None)
def calls():
    """every Call of the table but the largest one (largest_call), by name"""
    out = collections.OrderedDict()
    for c in _group_a() + _group_b() + _group_c() + _group_d() + _group_e() + _group_f() + _group_h() + _group_i():
        assert c.name not in out
        out[c.name] = c
    return out


def group(g):
    return [c for c in calls().values() if c.group == g]
