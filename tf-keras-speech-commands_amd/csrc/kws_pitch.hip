// csrc/kws_pitch.hip -- tempo and pitch perturbation of raw audio by a phase vocoder (include/kws.h: kws_pitch_workspace_bytes,
// kws_pitch_stft, kws_pitch_apply).
//
// Two kernels per tile of clips, 256 threads a block, the spectrum D[m][k] of a tile in the caller's workspace between them.
//   analysis:  a block transforms G = 1024 / (N/2) frames at once, N/8 threads a frame.  A frame's N windowed real samples are packed as
//              N/2 complex points; a Stockham FFT runs radix-4 passes (and one radix-2 pass when log2(N/2) is odd) with a thread's four
//              points in registers and two LDS buffers for the exchanges (padded every 16 points: the first pass stores at stride 4);
//              the first pass takes its points straight from the loads; the unpacking of the real FFT writes the N/2 + 1 bins.
//   synthesis: one block per clip.  Thread t owns the bins k = t, t + 256, ... and carries their phase from frame to frame in
//              registers; G output frames are synthesized into LDS, packed for the inverse real FFT, transformed by the same routine
//              (on conjugated data) and overlap-added by a thread per output sample in frame order -- no atomics, so two calls give
//              the same bits.  A chunk of G frames completes G N/4 samples; the 3 N/4 unfinished ones are carried in LDS.  A pitched
//              clip's stretched signal goes to the workspace and is then resampled by kws_resample.h's interpolation, with the
//              resampler's table in the LDS the vocoder has left; any other clip's goes straight to the output row.
// Twiddles and the window are made per block with sincospif / sinpif (2 N evaluations against 10 N log2 N flops per group of frames).
#include <cfloat>
#include <climits>
#include <cmath>
#include <type_traits>

#include "kws_common.h"
#include "kws_wave_stage.h"
#include "kws_device.h"
#include "kws_resample.h"

namespace kws {
namespace pv {

constexpr int kThreads = 256;
constexpr int kPoints = 1024;                            // complex points a block transforms at once
constexpr int kBuf = kPoints + kPoints / 16;             // float2 of one padded exchange buffer
constexpr int kMaxSamples = 1 << 20;
constexpr int kMaxZ = 32;                                // kws_resampler_create's limit on zero crossings
enum { kPvStretch = 0, kPvTempo = 1, kPvPitch = 2, kPvSemis = 3, kPvFields = 4 };   // draw fields: aug_hash(seed_p, step, 4 p + f)

// What a clip can need when no clip's rho exceeds rho_max and no clip's r exceeds r_max: floor((max_samples - 1) r) + 2 + ceil(Z max(r, 1))
// stretched samples (the last output's right wing), the output frames that reach them and the analysis frames those read.  Strides are
// multiples of 128 bytes.  The workspace is sized for the ranges' ends (rho = 4, r = 2, Z = 32: 2 max_samples + 64 samples); a call
// sizes its tiles for its own ranges, so a workspace for T clips holds more than T at a time unless the ranges are the widest.
struct Slots {
    int need_max, jn_max, mn_max;
    int64_t spec_stride, st_stride;                      // float2 / float per clip
    size_t clip_bytes;
};
static inline Slots slots(int N, int max_samples, double rho_max = 4.0, double r_max = 2.0, int Z = kMaxZ)
{
    Slots s;
    const int H = N / 4;
    s.need_max = (int)std::floor((double)(max_samples - 1) * r_max) + 2 + (int)std::ceil((double)Z * (r_max > 1.0 ? r_max : 1.0));
    s.jn_max = (s.need_max + N / 2 + H - 1) / H;
    s.mn_max = (int)std::floor((double)(s.jn_max - 1) * rho_max) + 2;
    s.spec_stride = (((int64_t)s.mn_max * (N / 2 + 1)) + 15) / 16 * 16;
    s.st_stride = ((int64_t)s.need_max + 31) / 32 * 32;
    s.clip_bytes = (size_t)s.spec_stride * sizeof(float2) + (size_t)s.st_stride * sizeof(float);
    return s;
}

struct PlanArgs {
    kws_pitch_params p;
    int Z;                                               // the resampler's zero crossings (0 without one)
    int64_t position_base;
    uint32_t step;
    int ex_t, ex_p;                                      // the host's values are staged in tempo_used / pitch_used
    float *tempo_used, *pitch_used;
    int need_cap, mn_cap;                                // what a slot of the workspace holds: no clip is planned beyond it
};

// What clip b gets: its draws, and how much of the vocoder its max_samples outputs need.
struct ClipPlan {
    int row, Ls, M, Jtot, lo, need, Jn, Mn;              // lo = L'; need: stretched samples; Jn, Mn: output / analysis frames needed
    float tempo, semis, r;
    double rho;
    bool vocoded;
};
template <int N>
__device__ __forceinline__ ClipPlan clip_plan(const int32_t *__restrict__ index, const int32_t *valid_len, int64_t stride, const PlanArgs &a, int b)
{
#pragma clang fp contract(off)
    constexpr int H = N / 4;
    ClipPlan c;
    const int ms = a.p.max_samples;
    const ClipSrc src = clip_src(index, valid_len, stride, ms, b);
    c.row = src.row;
    c.Ls = src.len;
    const uint32_t pos0 = aug_pos(a.position_base, b, kPvFields);
    float tempo = 0.f, semis = __builtin_nanf("");
    if (a.ex_t) tempo = a.tempo_used[b];
    else if (aug_unit(aug_hash(a.p.seed, a.step, pos0 + kPvStretch)) < a.p.tempo_rate)
        tempo = __fmaf_rn(aug_unit(aug_hash(a.p.seed, a.step, pos0 + kPvTempo)), a.p.tempo_hi - a.p.tempo_lo, a.p.tempo_lo);
    if (a.ex_p) semis = a.pitch_used[b];
    else if (aug_unit(aug_hash(a.p.seed, a.step, pos0 + kPvPitch)) < a.p.pitch_rate)
        semis = __fmaf_rn(aug_unit(aug_hash(a.p.seed, a.step, pos0 + kPvSemis)), a.p.pitch_hi - a.p.pitch_lo, a.p.pitch_lo);
    const bool pitched = !(semis != semis);
    c.tempo = tempo;
    c.semis = semis;
    c.vocoded = tempo != 0.f || pitched;
    c.r = pitched ? (float)exp2((double)semis / 12.0) : 1.f;
    c.rho = (double)(tempo != 0.f ? tempo : 1.f) / (double)c.r;
    c.M = 1 + c.Ls / H;
    c.lo = src.clipped;
    c.Jtot = c.need = c.Jn = c.Mn = 0;
    if (!c.vocoded) return c;
    const double Jd = ceil((double)c.M / c.rho), Lst = floor((double)c.Ls / c.rho + 0.5), rd = (double)c.r;
    c.Jtot = Jd < 1073741824.0 ? (int)Jd : 1073741824;
    double lo = c.r != 1.f ? ceil(Lst / rd) : Lst;
    lo = lo < (double)ms ? lo : (double)ms;
    c.lo = (int)lo;
    if (c.lo == 0) return c;
    double need = lo;
    if (c.r != 1.f) {                                    // the last output's right wing ends before n0 + 1 + Z / s
        const double s = rd > 1.0 ? 1.0 / rd : 1.0;
        need = floor((lo - 1.0) * rd) + 2.0 + ceil((double)a.Z / s);
        need = need < Lst ? need : Lst;
    }
    c.need = need < (double)a.need_cap ? (int)need : a.need_cap;
    const int jn = (c.need + N / 2 + H - 1) / H;         // the frames j with j H < need + N / 2
    c.Jn = jn < c.Jtot ? jn : c.Jtot;
    const double mn = floor((double)(c.Jn - 1) * c.rho) + 2.0;
    c.Mn = mn < (double)c.M ? (int)mn : c.M;
    c.Mn = c.Mn < a.mn_cap ? c.Mn : a.mn_cap;
    return c;
}

__device__ __forceinline__ int pad(int p) { return p + (p >> 4); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// forward 4-point DFT in place
__device__ __forceinline__ void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = csub(a1, a3);
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = make_float2(t1.x + t3.y, t1.y - t3.x);   // t1 - i t3
    a3 = make_float2(t1.x - t3.y, t1.y + t3.x);   // t1 + i t3
}

// tw[m] = exp(-2 pi i m / N), m < N; win[i] = sin^2(pi i / N) = 0.5 - 0.5 cos(2 pi i / N) without the cancellation near i = 0
template <int N>
__device__ __forceinline__ void make_tables(float2 *tw, float *win)
{
    for (int i = threadIdx.x; i < N; i += kThreads) {
        float s, c;
        sincospif((float)i * (2.0f / N), &s, &c);
        tw[i] = make_float2(c, -s);
        const float h = sinpif((float)i * (1.0f / N));
        win[i] = h * h;
    }
}

// The forward FFT of Nc complex points for each of the kPoints / Nc frames of a block.  Thread tid works on frame tid / T, T = Nc / 4, and
// enters with a[q] = x[lt + T q], lt = tid % T.  Stockham passes: the butterfly j of a pass with Ns finished points per sub-transform
// reads x[j + q Nc / 4], turns it by exp(-2 pi i q k / (4 Ns)), k = j % Ns, and writes bin q at (j - k) 4 + k + q Ns.  Returns the
// buffer that holds the bins in natural order (point n of frame f at pad(f Nc + n)); ends with a barrier.  The caller's barrier before
// the call frees b0.
template <int Nc>
__device__ __forceinline__ const float2 *fft_frames(float2 (&a)[4], float2 *b0, float2 *b1, const float2 *tw, int tid)
{
    constexpr int T = Nc / 4;
    const int lt = tid & (T - 1), base = (tid / T) * Nc;
    float2 *src = b1, *dst = b0;
    int Ns = 1;
#pragma unroll
    for (; Ns * 4 <= Nc; Ns *= 4) {
        const int k = lt & (Ns - 1);
        if (Ns > 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = src[pad(base + lt + T * q)];
            const int step = 2 * k * (Nc / (4 * Ns));     // index of exp(-2 pi i k / (4 Ns)) in the N-point table
            a[1] = cmul(a[1], tw[step]);
            a[2] = cmul(a[2], tw[2 * step]);
            a[3] = cmul(a[3], tw[3 * step]);
        }
        dft4(a[0], a[1], a[2], a[3]);
        const int o = base + ((lt - k) << 2) + k;
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[pad(o + q * Ns)] = a[q];
        __syncthreads();
        float2 *t = src;
        src = dst;
        dst = t;
    }
    if (Ns < Nc) {                                        // Nc = 2 Ns: one radix-2 pass
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = lt + T * i;
            const float2 u = src[pad(base + j)], v = cmul(src[pad(base + j + Nc / 2)], tw[2 * j]);
            dst[pad(base + j)] = cadd(u, v);
            dst[pad(base + j + Nc / 2)] = csub(u, v);
        }
        __syncthreads();
        return dst;
    }
    return src;
}

// bin k <= Nc of the real FFT from the packed transform Z (of frame base / Nc): E = (Z[k] + conj Z[Nc - k]) / 2,
// O = (Z[k] - conj Z[Nc - k]) / 2i, D = E + exp(-2 pi i k / N) O; bins 0 and Nc are real
template <int Nc>
__device__ __forceinline__ float2 unpack_bin(const float2 *Z, int base, int k, const float2 *tw)
{
    const float2 zk = Z[pad(base + (k & (Nc - 1)))], zm = Z[pad(base + ((Nc - k) & (Nc - 1)))];
    const float ex = 0.5f * (zk.x + zm.x), ey = 0.5f * (zk.y - zm.y), ox = 0.5f * (zk.y + zm.y), oy = -0.5f * (zk.x - zm.x);
    const float2 w = tw[k];
    float2 d = make_float2(ex + (w.x * ox - w.y * oy), ey + (w.x * oy + w.y * ox));
    if (k == 0 || k == Nc) d.y = 0.f;
    return d;
}

// LDS of both kernels: tw (N float2), two exchange buffers, win (N float), and for the synthesis the carry (3 N / 4 float)
template <int N>
constexpr int lds_bytes(bool synth) { return (N + 2 * kBuf) * (int)sizeof(float2) + (N + (synth ? 3 * N / 4 : 0)) * (int)sizeof(float); }

// D[m][k] of the frames m < limit of clip blockIdx.y: limit = the frames the clip's outputs need (planned, kws_pitch_apply) or `frames`
// (kws_pitch_stft; rows from the clip's own M on are zeros).  Block x takes the groups of G frames x, x + gridDim.x, ...
template <int N, typename WavT>
__global__ __launch_bounds__(kThreads) void pitch_stft_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                              const int32_t *__restrict__ valid_len, PlanArgs pa, int planned,
                                                              float2 *__restrict__ spec, int64_t clip_stride, int frames)
{
    constexpr int Nc = N / 2, H = N / 4, T = Nc / 4, G = kPoints / Nc, KB = Nc + 1;
    extern __shared__ float2 lds[];
    float2 *tw = lds, *b0 = tw + N, *b1 = b0 + kBuf;
    float *win = reinterpret_cast<float *>(b1 + kBuf);
    const int b = blockIdx.y, tid = threadIdx.x;
    int row, Ls, M, limit;
    if (planned) {
        const ClipPlan c = clip_plan<N>(index, valid_len, stride, pa, b);
        row = c.row, Ls = c.Ls, M = c.M, limit = c.Mn;
    } else {
        const ClipSrc src = clip_src(index, valid_len, stride, 1, b);
        row = src.row, Ls = src.len, M = 1 + Ls / H, limit = frames;
    }
    if ((int)blockIdx.x * G >= limit) return;
    make_tables<N>(tw, win);
    __syncthreads();
    const WavT *v = wav + (int64_t)row * stride;
    float2 *D = spec + (int64_t)b * clip_stride;
    const int f = tid / T, lt = tid & (T - 1);
    for (int g0 = blockIdx.x * G; g0 < limit; g0 += gridDim.x * G) {
        const int m = g0 + f;
        const bool live = m < limit && m < M;
        float2 a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 2 * (lt + T * q);
            const int64_t t = (int64_t)m * H + i - N / 2;
            const float x0 = live && t >= 0 && t < Ls ? aug_to_f32(v[t]) : 0.f;
            const float x1 = live && t + 1 >= 0 && t + 1 < Ls ? aug_to_f32(v[t + 1]) : 0.f;
            a[q] = make_float2(win[i] * x0, win[i + 1] * x1);
        }
        const float2 *Z = fft_frames<Nc>(a, b0, b1, tw, tid);
        if (m < limit) {
            float2 *Dm = D + (int64_t)m * KB;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lt + T * q;
                Dm[k] = live ? unpack_bin<Nc>(Z, f * Nc, k, tw) : make_float2(0.f, 0.f);
            }
            if (lt == 0) Dm[Nc] = live ? unpack_bin<Nc>(Z, f * Nc, Nc, tw) : make_float2(0.f, 0.f);
        }
        __syncthreads();                                 // the next group's first pass overwrites b0
    }
}

// x - 2 pi rint(x / 2 pi), the multiple taken off in two parts
__device__ __forceinline__ float wrap_pi(float x)
{
    const float n = rintf(x * 0.159154943091895336f);
    return __fmaf_rn(-n, -1.74845553e-7f, __fmaf_rn(-n, 6.28318548202514648f, x));
}

struct Polar {
    float ang, mag;
};
// |D[m][k]| and ang(D[m][k]); 0 and 0 for a frame past the clip's last (M: the frames the slot holds, which end there unless the outputs
// need fewer) and for a bin that is exactly zero
__device__ __forceinline__ Polar polar(const float2 *__restrict__ D, int m, int M, int KB, int k)
{
    Polar p = {0.f, 0.f};
    if (m < M) {
        const float2 z = D[(int64_t)m * KB + k];
        p.mag = sqrtf(__fmaf_rn(z.x, z.x, z.y * z.y));
        p.ang = z.x == 0.f && z.y == 0.f ? 0.f : atan2f(z.y, z.x);
    }
    return p;
}

template <int N, typename WavT>
__global__ __launch_bounds__(kThreads) void pitch_synth_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                               const int32_t *__restrict__ valid_len, PlanArgs pa,
                                                               const float *__restrict__ table, int P, const float2 *__restrict__ spec,
                                                               int64_t clip_stride, float *stretched, int64_t st_stride, float *out,
                                                               int64_t out_stride, int32_t *__restrict__ lengths)
{
    constexpr int Nc = N / 2, H = N / 4, T = Nc / 4, G = kPoints / Nc, KB = Nc + 1;
    constexpr int kBins = (KB + kThreads - 1) / kThreads, kSpan = (G + 3) * H, kPer = (kSpan + kThreads - 1) / kThreads;
    extern __shared__ float2 lds[];
    float2 *tw = lds, *b0 = tw + N, *b1 = b0 + kBuf;
    float *win = reinterpret_cast<float *>(b1 + kBuf), *carry = win + N;
    const int b = blockIdx.x, tid = threadIdx.x;
    const ClipPlan c = clip_plan<N>(index, valid_len, stride, pa, b);
    __syncthreads();                                     // every thread has read the staged values before thread 0 overwrites them
    if (tid == 0) {
        lengths[b] = c.lo;
        if (pa.tempo_used) pa.tempo_used[b] = c.tempo;
        if (pa.pitch_used) pa.pitch_used[b] = c.semis;
    }
    const WavT *v = wav + (int64_t)c.row * stride;
    float *dst = out + (int64_t)b * out_stride;
    if (!c.vocoded) {                                    // left as it is: the f32 conversion
        dry_copy<kThreads>(dst, v, c.lo, out_stride);
        return;
    }
    if (c.lo > 0) {
        const bool resampled = c.r != 1.f;
        float *st = resampled ? stretched + (int64_t)b * st_stride : dst;
        const float2 *D = spec + (int64_t)b * clip_stride;
        make_tables<N>(tw, win);
        for (int i = tid; i < 3 * H; i += kThreads) carry[i] = 0.f;
        __syncthreads();
        float phi[kBins];
        Polar d0[kBins], d1[kBins];
        int pm0 = -2;
        const int f = tid / T, lt = tid & (T - 1);
        for (int c0 = 0; c0 * H < c.need + N / 2; c0 += G) {
            // 1. the bins of the frames c0 .. c0 + G - 1, into b1 (frame g at g KB)
            for (int g = 0; g < G; ++g) {
                const int j = c0 + g;
                if (j >= c.Jn) {
                    for (int k = tid; k < KB; k += kThreads) b1[g * KB + k] = make_float2(0.f, 0.f);
                    continue;
                }
                int m0;
                float alpha;
                {
#pragma clang fp contract(off)
                    const double t = (double)j * c.rho, fl = floor(t);
                    m0 = (int)fl;
                    alpha = (float)(t - fl);
                }
#pragma unroll
                for (int i = 0; i < kBins; ++i) {
                    const int k = tid + i * kThreads;
                    if (k >= KB) continue;
                    if (m0 != pm0) {
                        d0[i] = m0 == pm0 + 1 ? d1[i] : polar(D, m0, c.Mn, KB, k);
                        d1[i] = polar(D, m0 + 1, c.Mn, KB, k);
                    }
                    if (j == 0) phi[i] = d0[i].ang;
                    const float mag = (1.f - alpha) * d0[i].mag + alpha * d1[i].mag;
                    float sn, cs;
                    sincosf(phi[i], &sn, &cs);
                    float2 y = make_float2(mag * cs, mag * sn);
                    const int q = ((j & 3) * (k & 3)) & 3;                  // times i^(j k)
                    if (q == 1) y = make_float2(-y.y, y.x);
                    else if (q == 2) y = make_float2(-y.x, -y.y);
                    else if (q == 3) y = make_float2(y.y, -y.x);
                    b1[g * KB + k] = y;
                    // The measured advance minus the quarter turns of (pi / 2) k that are no whole turn, wrapped into [-pi, pi], in
                    // fp64 and rounded once.  In fp32 the difference of the angles minus kq fl(pi / 2) lands on a grid of 2^-22 or
                    // 2^-21, which swallows a low part of pi / 2 (4.4e-8): every bin with k mod 4 != 0 then ran 4.4e-8 kq rad a frame
                    // fast, the same way in every frame: 3e-5 rad after a second at N = 256, and a steady tone shows it.
                    double dd = (double)d1[i].ang - (double)d0[i].ang - (double)(k & 3) * 1.5707963267948966;
                    dd -= 6.283185307179586 * rint(dd * 0.15915494309189535);
                    phi[i] = wrap_pi(phi[i] + (float)dd);
                }
                pm0 = m0;
            }
            __syncthreads();
            // 2. packed for the inverse real FFT: Z'[k] = (Y[k] + conj Y[Nc - k]) + i exp(2 pi i k / N) (Y[k] - conj Y[Nc - k]); its
            // inverse transform is conj(FFT(conj Z')), and y[2n] + i y[2n + 1] = z[n] / N
            float2 a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lt + T * q;
                float2 yk = b1[f * KB + k], ym = b1[f * KB + Nc - k];
                if (k == 0) yk.y = 0.f, ym.y = 0.f;                        // bins 0 and N / 2 count with their real parts
                const float2 A = make_float2(yk.x + ym.x, yk.y - ym.y), B = make_float2(yk.x - ym.x, yk.y + ym.y);
                const float2 w = tw[k];
                const float2 wB = cmul(make_float2(w.x, -w.y), B);
                a[q] = make_float2(A.x - wB.y, -(A.y + wB.x));
            }
            const float2 *X = fft_frames<Nc>(a, b0, b1, tw, tid);
            // 3. overlap-add: sample p of the chunk = carry + sum over g ascending of w[p - g H] y_g[p - g H]
            float val[kPer];
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int p = tid + i * kThreads;
                float s = 0.f;
                if (p < kSpan) {
                    if (p < 3 * H) s = carry[p];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const int i0 = p - g * H;
                        if (i0 >= 0 && i0 < N) {
                            const float2 z = X[pad(g * Nc + (i0 >> 1))];
                            s = __fmaf_rn(win[i0], ((i0 & 1) ? -z.y : z.x) * (1.0f / N), s);
                        }
                    }
                }
                val[i] = s;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int p = tid + i * kThreads;
                if (p < G * H) {
                    const int pp = c0 * H + p, sidx = pp - N / 2;          // position with and without the leading N / 2
                    if (sidx >= 0 && sidx < c.need) {
                        const int jhi = pp / H < c.Jtot - 1 ? pp / H : c.Jtot - 1;
                        float wss = 0.f;
                        for (int jj = pp >= N ? (pp - N) / H + 1 : 0; jj <= jhi; ++jj) wss = __fmaf_rn(win[pp - jj * H], win[pp - jj * H], wss);
                        st[sidx] = wss > 1e-8f ? val[i] / wss : val[i];
                    }
                } else if (p < kSpan)
                    carry[p - G * H] = val[i];
            }
            __syncthreads();
        }
        if (resampled) {                                 // the stretched signal played r times faster (kws_resample.h)
            float *h = reinterpret_cast<float *>(lds);
            const int n_table = pa.Z * P + 1;
            for (int i = tid; i < n_table; i += kThreads) h[i] = table[i];
            __syncthreads();
            const double rd = (double)c.r, s = rd > 1.0 ? 1.0 / rd : 1.0, dP = (double)P, lim = (double)(pa.Z * P);
            const float sf = (float)s;
            for (int n = tid; n < c.lo; n += kThreads) dst[n] = spd::resample_at<float>(st, h, n, c.need, rd, s, sf, dP, lim);
        }
    }
    for (int64_t t = (int64_t)c.lo + tid; t < out_stride; t += kThreads) dst[t] = 0.f;
}

template <typename F>
inline int for_n_fft(int n_fft, F &&f)
{
    return n_fft == 256 ? f(std::integral_constant<int, 256>{}) : n_fft == 512 ? f(std::integral_constant<int, 512>{}) : f(std::integral_constant<int, 1024>{});
}

static inline int check_n_fft(int n_fft)
{
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return fail(KWS_ERR_INVALID, "n_fft %d is none of 256, 512, 1024", n_fft);
    return KWS_OK;
}

// blocks along the frames: two groups of frames a block for a clip that fills its row
static inline unsigned frame_blocks(int frames, int N)
{
    const int G = kPoints / (N / 2), groups = (frames + G - 1) / G;
    return (unsigned)(groups > 1 ? (groups + 1) / 2 : 1);
}

}  // namespace pv
}  // namespace kws

using namespace kws;
using namespace kws::pv;

extern "C" {

int kws_pitch_workspace_bytes(int n_fft, int max_samples, int tile_clips, size_t *bytes)
{
    if (!bytes) return fail(KWS_ERR_INVALID, "null argument");
    *bytes = 0;
    if (int rc = check_n_fft(n_fft)) return rc;
    if (max_samples < 1) return fail(KWS_ERR_INVALID, "max_samples must be >= 1");
    if (max_samples > kMaxSamples) return fail(KWS_ERR_UNSUPPORTED, "max_samples %d > %d", max_samples, kMaxSamples);
    if (tile_clips < 1) return fail(KWS_ERR_INVALID, "tile_clips must be >= 1, got %d", tile_clips);
    *bytes = slots(n_fft, max_samples).clip_bytes * (size_t)tile_clips;
    return KWS_OK;
}

int kws_pitch_stft(const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride, const int32_t *valid_len, int n_fft,
                   float *out, int frames, void *stream)
{
    if (B > 0 && (!wav || !out)) return fail(KWS_ERR_INVALID, "null argument");
    if (int rc = check_n_fft(n_fft)) return rc;
    if (frames < 1) return fail(KWS_ERR_INVALID, "frames must be >= 1, got %d", frames);
    if (int rc = check_clip_batch(1, INT_MAX, B, stride, true, valid_len, 0, nullptr, wav_dtype)) return rc;
    if (B == 0) return KWS_OK;
    int dev = 0;
    KWS_HIP_CHECK(hipGetDevice(&dev));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PlanArgs pa = {};
    const int64_t clip_stride = (int64_t)frames * (n_fft / 2 + 1);
    return for_n_fft(n_fft, [&](auto nn) -> int {
        constexpr int N = decltype(nn)::value;
        return for_wav_type(wav_dtype, "pitch_stft_f32", "pitch_stft_i16", [&](auto t, const char *name) -> int {
            using WavT = decltype(t);
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pitch_stft_kernel<N, WavT>), lds_bytes<N>(false))) return rc;
            for (int b0 = 0; b0 < B; b0 += 32768) {
                const int n = B - b0 < 32768 ? B - b0 : 32768;
                // without an index clip b is row b: the tile's rows start at b0
                const WavT *w = static_cast<const WavT *>(wav) + (index ? 0 : (int64_t)b0 * stride);
                const int32_t *vl = valid_len && !index ? valid_len + b0 : valid_len;
                KWS_LAUNCH(name, (pitch_stft_kernel<N, WavT>), dim3(frame_blocks(frames, N), (unsigned)n), dim3(kThreads), lds_bytes<N>(false), s,
                           w, stride, index ? index + b0 : nullptr, vl, pa, 0, reinterpret_cast<float2 *>(out) + (int64_t)b0 * clip_stride,
                           clip_stride, frames);
                KWS_LAUNCH_CHECK("pitch_stft_kernel");
            }
            return KWS_OK;
        });
    });
}

int kws_pitch_apply(const kws_resampler *rs, const kws_pitch_params *p, const void *wav, int wav_dtype, const int32_t *index, int B,
                    int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const float *explicit_tempo,
                    const float *explicit_semitones, float *out, int64_t out_stride, int32_t *lengths, float *tempo_used, float *pitch_used,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (!p || (B > 0 && (!wav || !out || !lengths))) return fail(KWS_ERR_INVALID, "null argument");
    if (!(p->tempo_rate >= 0.f && p->tempo_rate <= 1.f)) return fail(KWS_ERR_INVALID, "tempo_rate %g is outside [0, 1]", (double)p->tempo_rate);
    if (!(p->pitch_rate >= 0.f && p->pitch_rate <= 1.f)) return fail(KWS_ERR_INVALID, "pitch_rate %g is outside [0, 1]", (double)p->pitch_rate);
    if (p->tempo_rate > 0.f && !(0.5f <= p->tempo_lo && p->tempo_lo <= p->tempo_hi && p->tempo_hi <= 2.f))
        return fail(KWS_ERR_INVALID, "tempo range [%g, %g] needs 0.5 <= lo <= hi <= 2", (double)p->tempo_lo, (double)p->tempo_hi);
    if (p->pitch_rate > 0.f && !(-12.f <= p->pitch_lo && p->pitch_lo <= p->pitch_hi && p->pitch_hi <= 12.f))
        return fail(KWS_ERR_INVALID, "pitch range [%g, %g] semitones needs -12 <= lo <= hi <= 12", (double)p->pitch_lo, (double)p->pitch_hi);
    if (int rc = check_n_fft(p->n_fft)) return rc;
    if (int rc = check_clip_batch(p->max_samples, kMaxSamples, B, stride, true, valid_len, position_base, &out_stride, wav_dtype)) return rc;
    if (B > 0 && (const void *)out == wav) return fail(KWS_ERR_INVALID, "the perturbation cannot run in place (out == wav)");
    // the ends of this call's ranges: what its clips can need of the workspace
    bool vocodes = (!explicit_tempo && p->tempo_rate > 0.f) || (!explicit_semitones && p->pitch_rate > 0.f);
    bool needs_table = !explicit_semitones && p->pitch_rate > 0.f;
    float tempo_max = !explicit_tempo && p->tempo_rate > 0.f && p->tempo_hi > 1.f ? p->tempo_hi : 1.f;
    float n_lo = needs_table && p->pitch_lo < 0.f ? p->pitch_lo : 0.f, n_hi = needs_table && p->pitch_hi > 0.f ? p->pitch_hi : 0.f;
    if (explicit_tempo) {
        if (!tempo_used && B > 0) return fail(KWS_ERR_INVALID, "explicit_tempo needs tempo_used (the ratios are staged there)");
        for (int b = 0; b < B; ++b) {
            if (explicit_tempo[b] != 0.f && !(explicit_tempo[b] >= 0.5f && explicit_tempo[b] <= 2.f))
                return fail(KWS_ERR_INVALID, "clip %d: tempo %g is neither 0 nor in [0.5, 2]", b, (double)explicit_tempo[b]);
            vocodes = vocodes || explicit_tempo[b] != 0.f;
            tempo_max = explicit_tempo[b] > tempo_max ? explicit_tempo[b] : tempo_max;
        }
    }
    if (explicit_semitones) {
        if (!pitch_used && B > 0) return fail(KWS_ERR_INVALID, "explicit_semitones needs pitch_used (the shifts are staged there)");
        for (int b = 0; b < B; ++b) {
            if (std::isnan(explicit_semitones[b])) continue;
            if (!(explicit_semitones[b] >= -12.f && explicit_semitones[b] <= 12.f))
                return fail(KWS_ERR_INVALID, "clip %d: shift %g semitones is neither NaN nor in [-12, 12]", b, (double)explicit_semitones[b]);
            needs_table = true;
            n_lo = explicit_semitones[b] < n_lo ? explicit_semitones[b] : n_lo;
            n_hi = explicit_semitones[b] > n_hi ? explicit_semitones[b] : n_hi;
        }
    }
    vocodes = vocodes || needs_table;
    if (!rs && needs_table) return fail(KWS_ERR_INVALID, "a pitch shift needs a resampler (the interpolation table)");
    if (B == 0) return KWS_OK;
    // r is monotone in n and computed as on the device, so these are the largest rho and r of any clip
    const double r_min = (double)(float)std::exp2((double)n_lo / 12.0), r_max = (double)(float)std::exp2((double)n_hi / 12.0);
    const Slots sl = slots(p->n_fft, p->max_samples, (double)tempo_max / r_min, r_max, rs ? rs->Z : 0);
    int tile = B;
    if (vocodes) {
        if (!workspace) return fail(KWS_ERR_INVALID, "null workspace");
        const size_t one = slots(p->n_fft, p->max_samples).clip_bytes, fit = workspace_bytes / sl.clip_bytes;
        if (workspace_bytes < one) return fail(KWS_ERR_WORKSPACE, "a workspace of %zu bytes holds no clip (one needs %zu)", workspace_bytes, one);
        tile = fit < 32768 ? (int)fit : 32768;
        const int n_tiles = (B + tile - 1) / tile;       // equal tiles: a short last one would leave compute units idle (a block per clip)
        tile = (B + n_tiles - 1) / n_tiles;
    }
    int dev = 0;
    KWS_HIP_CHECK(hipGetDevice(&dev));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *table = nullptr;
    size_t table_bytes = 0;
    if (rs) {
        if (int rc = spd::device_table(rs, &table)) return rc;
        table_bytes = sizeof(float) * rs->table.size();
    }
    if (explicit_tempo) KWS_HIP_CHECK(hipMemcpyAsync(tempo_used, explicit_tempo, sizeof(float) * B, hipMemcpyHostToDevice, s));
    if (explicit_semitones) KWS_HIP_CHECK(hipMemcpyAsync(pitch_used, explicit_semitones, sizeof(float) * B, hipMemcpyHostToDevice, s));
    const int N0 = p->n_fft, Z = rs ? rs->Z : 0, P = rs ? rs->P : 0;
    // the frames of a clip that fills its row, at most what a slot holds
    const int64_t row_frames = 1 + stride / (N0 / 4);
    const int frames = row_frames < sl.mn_max ? (int)row_frames : sl.mn_max;
    float2 *spec = static_cast<float2 *>(workspace);
    return for_n_fft(N0, [&](auto nn) -> int {
        constexpr int N = decltype(nn)::value;
        return for_wav_type(wav_dtype, "pitch_stft_f32", "pitch_stft_i16", [&](auto t, const char *name) -> int {
            using WavT = decltype(t);
            const char *synth_name = std::is_same<WavT, float>::value ? "pitch_synth_f32" : "pitch_synth_i16";
            const int lds_a = lds_bytes<N>(false);
            const int lds_s = lds_bytes<N>(true) > (int)table_bytes ? lds_bytes<N>(true) : (int)table_bytes;
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pitch_stft_kernel<N, WavT>), lds_a)) return rc;
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pitch_synth_kernel<N, WavT>), lds_s)) return rc;
            for (int b0 = 0; b0 < B; b0 += tile) {
                const int n = B - b0 < tile ? B - b0 : tile;
                // without an index clip b is row b: the tile's rows start at b0
                const WavT *w = static_cast<const WavT *>(wav) + (index ? 0 : (int64_t)b0 * stride);
                const int32_t *vl = valid_len && !index ? valid_len + b0 : valid_len, *ix = index ? index + b0 : nullptr;
                PlanArgs pa = {*p, Z, position_base + b0, (uint32_t)step, explicit_tempo ? 1 : 0, explicit_semitones ? 1 : 0,
                               tempo_used ? tempo_used + b0 : nullptr, pitch_used ? pitch_used + b0 : nullptr, sl.need_max, sl.mn_max};
                float *st = reinterpret_cast<float *>(spec + (int64_t)tile * sl.spec_stride);
                if (vocodes) {
                    KWS_LAUNCH(name, (pitch_stft_kernel<N, WavT>), dim3(frame_blocks(frames, N), (unsigned)n), dim3(kThreads), lds_a, s, w,
                               stride, ix, vl, pa, 1, spec, sl.spec_stride, 0);
                    KWS_LAUNCH_CHECK("pitch_stft_kernel");
                }
                KWS_LAUNCH(synth_name, (pitch_synth_kernel<N, WavT>), dim3((unsigned)n), dim3(kThreads), lds_s, s, w, stride, ix, vl, pa, table, P,
                           spec, sl.spec_stride, vocodes ? st : nullptr, sl.st_stride, out + (int64_t)b0 * out_stride, out_stride, lengths + b0);
                KWS_LAUNCH_CHECK("pitch_synth_kernel");
            }
            return KWS_OK;
        });
    });
}

}  // extern "C"
