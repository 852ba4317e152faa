"""float64 numpy restatement of the tempo and pitch perturbation (include/kws.h: kws_pitch_stft, kws_pitch_apply) for
tests/test_pitch_host.py and tests/test_pitch_gpu.py: the draws, the analysis, the phase vocoder, the overlap-add and, through
tests/speed_ref.py, the pitch shift's resampling.  Next to every frame it returns S = sum |w v| and next to every output sample
A[n] = the windowed, normalised sum of the bin magnitudes (carried through the resampler's sum |w| |v| for a pitched clip) and the tap
count T[n], which the float32 error bounds of the GPU tests are made of."""
import math

import numpy as np

import speed_ref as sr
from aug_ref import np_hash, np_unit

MIX = 0x8EBC6AF09C88C6E3
N_FFTS = (256, 512, 1024)
U = 2.0 ** -24
_I_POW = np.array([1.0, 1.0j, -1.0, -1.0j])


def np_draws(seed, step, pos, tempo_rate=0.0, tempo=(1.0, 1.0), pitch_rate=0.0, pitch=(0.0, 0.0)):
    """-> (stretched bool, tempo float32, pitched bool, semitones float32) per clip at the global positions pos, seed = WaveAugment's"""
    seed_p = seed ^ MIX
    pos = np.asarray(pos, np.uint64)
    u = [np_unit(np_hash(seed_p, step, np.uint64(4) * pos + np.uint64(f))) for f in range(4)]
    lo, hi = np.float32(tempo[0]), np.float32(tempo[1])
    plo, phi = np.float32(pitch[0]), np.float32(pitch[1])
    return (u[0] < np.float32(tempo_rate), sr._fmaf(u[1], hi - lo, lo), u[2] < np.float32(pitch_rate), sr._fmaf(u[3], phi - plo, plo))


def ratio(semitones):
    """r of a pitched clip (float32); 1 for NaN"""
    n = np.float32(semitones)
    return np.float32(1.0) if np.isnan(n) else np.float32(2.0 ** (float(n) / 12.0))


def rho(tempo, semitones):
    """the vocoder's rate (float64): tempo 0 = not stretched, semitones NaN = not pitched"""
    t = np.float32(tempo)
    return float(t if t != 0 else np.float32(1.0)) / float(ratio(semitones))


def window(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def n_frames(Ls, N):
    return 1 + Ls // (N // 4)


def stretch_length(Ls, rate):
    return int(math.floor(Ls / rate + 0.5))


def stft(v, N):
    """-> (D (M, N/2 + 1) complex128, S (M,) = sum_i |w_i v_i| per frame) of the clip v (1-D, its whole valid length)"""
    v = np.asarray(v, np.float64)
    Ls, H = len(v), N // 4
    M = n_frames(Ls, N)
    x = np.concatenate([np.zeros(N // 2), v, np.zeros(N + H)])
    fr = x[np.arange(M)[:, None] * H + np.arange(N)[None, :]] * window(N)[None, :]
    return np.fft.rfft(fr, axis=1), np.abs(fr).sum(1)


def _ang(z):
    a = np.arctan2(z.imag, z.real)
    a[(z.real == 0) & (z.imag == 0)] = 0.0
    return a


def vocoder(D, Ls, rate, N):
    """-> (y (Lst,), A (Lst,), J): the spectrum D (M, N/2 + 1) of a clip of Ls samples stretched at `rate` (float64)"""
    D = np.asarray(D, np.complex128)
    M, K = D.shape
    H = N // 4
    assert K == N // 2 + 1 and M == n_frames(Ls, N)
    J = int(math.ceil(M / rate))
    Dp = np.vstack([D, np.zeros((2, K), np.complex128)])
    k = np.arange(K)
    w = window(N)
    c = np.full(K, 2.0)
    c[0] = c[-1] = 1.0
    out, A, wss = (np.zeros((J - 1) * H + N) for _ in range(3))
    phi = _ang(Dp[0])
    for j in range(J):
        t = j * rate
        m0 = int(math.floor(t))
        al = t - m0
        d0, d1 = Dp[m0], Dp[m0 + 1]
        mag = (1.0 - al) * np.abs(d0) + al * np.abs(d1)
        Y = mag * _I_POW[(j * k) % 4] * np.exp(1j * phi)
        out[j * H:j * H + N] += w * np.fft.irfft(Y, N)
        A[j * H:j * H + N] += w * ((c * mag).sum() / N)
        wss[j * H:j * H + N] += w * w
        dl = _ang(d1) - _ang(d0) - (np.pi / 2.0) * k
        phi = phi + (dl - 2.0 * np.pi * np.rint(dl / (2.0 * np.pi)))
    nz = wss > 1e-8
    out[nz] /= wss[nz]
    A[nz] /= wss[nz]
    Lst = stretch_length(Ls, rate)
    assert N // 2 + Lst <= len(out)
    return out[N // 2:N // 2 + Lst], A[N // 2:N // 2 + Lst], J


def out_length(Ls, tempo, semitones, max_samples):
    """L' of a clip that is stretched or pitched"""
    Lst = stretch_length(Ls, rho(tempo, semitones))
    r = ratio(semitones)
    return min(Lst, max_samples) if r == 1 else sr.out_length(Lst, r, max_samples)


def perturb(v, tempo, semitones, max_samples, N=512, h=None, zero_crossings=16, phases=512, D=None):
    """one clip: -> dict(y float64 (L'), A, T, J) with tempo = 0 for "not stretched" and semitones = NaN for "not pitched"; D: the
    spectrum to run the vocoder on instead of stft(v) (the GPU's own, taken into float64)"""
    v = np.asarray(v, np.float64)
    if float(tempo) == 0.0 and np.isnan(semitones):
        y = v[:max_samples].copy()
        return dict(y=y, A=np.abs(y), T=np.zeros(len(y), np.int64), J=0)
    if D is None:
        D = stft(v, N)[0]
    y, A, J = vocoder(D, len(v), rho(tempo, semitones), N)
    r = ratio(semitones)
    if r == 1:
        y, A = y[:max_samples], A[:max_samples]
        return dict(y=y, A=A, T=np.zeros(len(y), np.int64), J=J)
    y2, _, T = sr.resample(y, r, max_samples, h, zero_crossings, phases)
    _, A2, _ = sr.resample(A, r, max_samples, h, zero_crossings, phases)
    return dict(y=y2, A=A2, T=T, J=J)
