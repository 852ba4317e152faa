// csrc/kws_filter.hip -- filter bank and the apply kernel of the Butterworth filter augmentation (include/kws.h: kws_filter_bank_*,
// kws_filter_apply; the filtfilt of tools/audio_process/wav_filter.py of the reference).
//
// One wave (a 64-thread block) per clip.  The cascade of S second-order sections (transposed direct form II, as scipy's sosfilt) is one
// linear system with n = 2 S states: s' = A s + B x.  A pass over the padded clip (Lv + 2 padlen samples) splits it into 64 chunks of
// C = 2^m samples, lane i owning chunk i:
//   1. every lane runs its chunk from a zero state (lane 0 from the pass's true initial state) and keeps the final state f_i;
//   2. an inclusive scan across lanes, F_i = A^C F_(i-1) + f_i, in log2(64) = 6 steps of __shfl_up and one n x n product with
//      A^(C 2^j) each, gives every chunk's true final state, and so (one lane up) its true initial state;
//   3. every lane reruns its chunk from the true state and writes the output.
// The recurrence, the scan and the bank run in fp64 (fp32 coefficients and states missed the featurizer suite's tolerance for a 50 Hz
// highpass: DESIGN section 11); samples are fp32 in memory.  The forward output goes to out[0, Lv) and, for the two odd-extension edges, to one LDS float per lane; the backward pass reads it
// reversed by index arithmetic and writes the result over it.  The edges are read into LDS before any write, so the clip may be filtered
// in place.  Sums are fp32 per lane and fp64 across the wave in a fixed order (no atomics), so two calls give the same bits.
#include <cfloat>
#include <cmath>
#include <vector>

#include "kws_common.h"
#include "kws_wave_stage.h"
#include "kws_device.h"
#include "kws_filter.h"

namespace kws {
namespace flt {

enum { kFltApply = 0, kFltFilter = 1, kFltFields = 2 };    // draw fields: aug_hash(seed_f, step, 2 p + f)

// one sample through the cascade; c[s] = (b0, b1, b2, -a1, -a2)
template <int S>
__device__ __forceinline__ double cascade(double x, double (&z)[2 * S], const double (&c)[S][5])
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double y = fma(c[s][0], x, z[2 * s]);
        z[2 * s] = fma(c[s][3], y, fma(c[s][1], x, z[2 * s + 1]));
        z[2 * s + 1] = fma(c[s][4], y, c[s][2] * x);
        x = y;
    }
    return x;
}

// Steps 2 of a pass: on entry z = f_i (lane 0: its true final state), on return z = the true initial state of chunk i (lane 0: s0).
template <int S>
__device__ __forceinline__ void chunk_scan(double (&z)[2 * S], const double (&s0)[2 * S], const double *__restrict__ pw, int m, int lane)
{
    constexpr int n = 2 * S;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int d = 1 << j;
        const double *P = pw + (m + j) * kMat;            // A^(2^(m + j)) = A^(C d)
        double o[n];
#pragma unroll
        for (int q = 0; q < n; ++q) o[q] = __shfl_up(z[q], d, kLanes);
        if (lane >= d) {
#pragma unroll
            for (int r = 0; r < n; ++r) {
                double acc = z[r];
#pragma unroll
                for (int q = 0; q < n; ++q) acc = fma(P[r * n + q], o[q], acc);
                z[r] = acc;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < n; ++q) {
        const double up = __shfl_up(z[q], 1, kLanes);
        z[q] = lane == 0 ? s0[q] : up;
    }
}

template <int S, typename WavT>
__global__ __launch_bounds__(64) void filter_apply_kernel(const WavT *wav, int64_t stride, const int32_t *__restrict__ index,
                                                          const int32_t *valid_len, kws_filter_params p, int K,
                                                          const double *__restrict__ table, const int32_t *__restrict__ padlens,
                                                          int64_t position_base, uint32_t step, int explicit_filter, float *out,
                                                          int64_t out_stride, int32_t *lengths, int32_t *filter_used)
{
    constexpr int n = 2 * S;
    __shared__ float edge[kLanes];                          // ext[0, padlen) then ext[padlen + Lv, Lv + 2 padlen); later y_fwd there
    const int b = blockIdx.x, lane = threadIdx.x;
    const ClipSrc src = clip_src(index, valid_len, stride, p.max_samples, b);
    const int lv = src.clipped;

    // the host's choices are staged in `filter_used` by kws_filter_apply
    int k = explicit_filter ? filter_used[b]
                            : aug_pick(p.seed, step, aug_pos(position_base, b, kFltFields), kFltApply, kFltFilter, p.filter_rate, K);
    k = __builtin_amdgcn_readfirstlane(k);
    const int padlen = k >= 0 ? padlens[k] : 0;
    if (lv <= padlen) k = -1;                               // too short for the odd extension (scipy raises): dry
    // in place, `wav` and `out` are one buffer: no __restrict__ on either
    const WavT *v = wav + (int64_t)src.row * stride;
    float *dst = out + (int64_t)b * out_stride;
    __syncthreads();                                        // every lane has read valid_len / filter_used before lane 0 overwrites them
    if (lane == 0) {
        lengths[b] = lv;
        if (filter_used) filter_used[b] = k;
    }
    if (k < 0) {                                            // dry: the f32 conversion
        dry_copy<kLanes>(dst, v, lv, out_stride);
        return;
    }

    const double *F = table + (int64_t)k * kStride;
    double c[S][5], zi[n];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int i = 0; i < 5; ++i) c[s][i] = F[5 * s + i];
#pragma unroll
    for (int q = 0; q < n; ++q) zi[q] = F[5 * S + q];
    const double *pw = F + kCoef;

    const int lpad = lv + 2 * padlen;
    int m = kMinLog;
    while ((kLanes << m) < lpad) ++m;
    const int C = 1 << m, t0 = lane * C;

    // the odd extension's edges, before any write (in place they are samples of the clip itself)
    const float v0 = aug_to_f32(v[0]), vl = aug_to_f32(v[lv - 1]);
    if (lane < padlen) {
        edge[lane] = 2.f * v0 - aug_to_f32(v[padlen - lane]);
        edge[padlen + lane] = 2.f * vl - aug_to_f32(v[lv - 2 - lane]);
    }
    __syncthreads();

    // ---- forward pass over ext[t], t < lpad ----
    auto ext = [&](int t) -> float {
        const int u = t - padlen;
        return (u >= 0 && u < lv) ? aug_to_f32(v[u]) : edge[u < 0 ? t : t - lv];
    };
    double s0[n], z[n];
    const double x0 = edge[0];
#pragma unroll
    for (int q = 0; q < n; ++q) {
        s0[q] = zi[q] * x0;
        z[q] = lane == 0 ? s0[q] : 0.f;
    }
    float ev = 0.f;
    for (int i = 0; i < C; ++i) {
        const int t = t0 + i;
        if (t < lpad) {
            const int u = t - padlen;
            const float x = ext(t);
            if (u >= 0 && u < lv) ev = fmaf(x, x, ev);
            (void)cascade<S>((double)x, z, c);
        }
    }
    chunk_scan<S>(z, s0, pw, m, lane);
    for (int i = 0; i < C; ++i) {
        const int t = t0 + i;
        if (t < lpad) {
            const int u = t - padlen;
            const float y = (float)cascade<S>((double)ext(t), z, c);
            if (u >= 0 && u < lv) dst[u] = y;
            else edge[u < 0 ? t : t - lv] = y;
        }
    }
    __syncthreads();                                        // the forward output is visible to every lane

    // ---- backward pass over w[t] = y_fwd[lpad - 1 - t] ----
    const double w0 = edge[2 * padlen - 1];
#pragma unroll
    for (int q = 0; q < n; ++q) {
        s0[q] = zi[q] * w0;
        z[q] = lane == 0 ? s0[q] : 0.f;
    }
    auto rev = [&](int t) -> float {
        const int r = lpad - 1 - t, u = r - padlen;
        return (u >= 0 && u < lv) ? dst[u] : edge[u < 0 ? r : r - lv];
    };
    for (int i = 0; i < C; ++i) {
        const int t = t0 + i;
        if (t < lpad) (void)cascade<S>((double)rev(t), z, c);
    }
    chunk_scan<S>(z, s0, pw, m, lane);
    float ey = 0.f;
    for (int i = 0; i < C; ++i) {
        const int t = t0 + i;
        if (t < lpad) {
            const int u = lpad - 1 - t - padlen;
            const float y = (float)cascade<S>((double)rev(t), z, c);
            if (u >= 0 && u < lv) {
                dst[u] = y;
                ey = fmaf(y, y, ey);
            }
        }
    }
    const double Ev = wave_sum((double)ev), Ey = wave_sum((double)ey);
    __syncthreads();                                        // the backward output is visible to every lane
    if (p.rescale) {
        const float scale = (float)sqrt(Ev / (Ey + (double)lv * (double)FLT_EPSILON));
        for (int t = lane; t < lv; t += kLanes) dst[t] *= scale;
    }
    for (int64_t t = (int64_t)lv + lane; t < out_stride; t += kLanes) dst[t] = 0.f;
}

template <int S>
int launch(const kws_filter_bank *fb, const kws_filter_params *p, const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride,
           const int32_t *valid_len, int64_t position_base, int64_t step, int explicit_filter, float *out, int64_t out_stride,
           int32_t *lengths, int32_t *filter_used, hipStream_t s)
{
    const dim3 grid((unsigned)B), block(kLanes);
    return for_wav_type(wav_dtype, "filter_apply_f32", "filter_apply_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        KWS_LAUNCH(name, (filter_apply_kernel<S, WavT>), grid, block, 0, s, static_cast<const WavT *>(wav), stride, index, valid_len, *p,
                   fb->K, fb->table, fb->d_padlen, position_base, (uint32_t)step, explicit_filter, out, out_stride, lengths, filter_used);
        KWS_LAUNCH_CHECK("filter_apply_kernel");
        return KWS_OK;
    });
}

// one zero-input step of the cascade (the kernel's recurrence in fp64): s' = A s
void host_step(const std::vector<double> &c, int S, std::vector<double> &z)
{
    double x = 0.0;
    for (int s = 0; s < S; ++s) {
        const double *cs = &c[5 * s];
        const double y = cs[0] * x + z[2 * s];
        z[2 * s] = cs[1] * x + z[2 * s + 1] + cs[3] * y;
        z[2 * s + 1] = cs[2] * x + cs[4] * y;
        x = y;
    }
}

}  // namespace flt
}  // namespace kws

using namespace kws;
using namespace kws::flt;

extern "C" {

int kws_filter_bank_create(const double *sos, int n_sections, const int32_t *padlen, int K, kws_filter_bank **out)
{
    if (!out || !sos || !padlen) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (K < 1) return fail(KWS_ERR_INVALID, "a filter bank needs at least one filter");
    if (n_sections < 1) return fail(KWS_ERR_INVALID, "n_sections must be >= 1, got %d", n_sections);
    if (n_sections > KWS_FILTER_MAX_SECTIONS)
        return fail(KWS_ERR_UNSUPPORTED, "%d sections > %d (KWS_FILTER_MAX_SECTIONS)", n_sections, KWS_FILTER_MAX_SECTIONS);
    const int S = n_sections, n = 2 * S;
    std::vector<double> table((size_t)K * kStride, 0.0);
    for (int k = 0; k < K; ++k) {
        if (padlen[k] < 1 || padlen[k] > KWS_FILTER_MAX_PADLEN)
            return fail(KWS_ERR_INVALID, "filter %d: padlen %d is outside [1, %d]", k, padlen[k], KWS_FILTER_MAX_PADLEN);
        // normalised coefficients (b0, b1, b2, -a1, -a2) / a0 per section
        std::vector<double> c(5 * S);
        for (int s = 0; s < S; ++s) {
            const double *q = sos + ((size_t)k * S + s) * 6;
            for (int i = 0; i < 6; ++i)
                if (!std::isfinite(q[i])) return fail(KWS_ERR_INVALID, "filter %d section %d: coefficient %d is not finite", k, s, i);
            if (q[3] == 0.0) return fail(KWS_ERR_INVALID, "filter %d section %d: a0 is 0", k, s);
            const double a1 = q[4] / q[3], a2 = q[5] / q[3];
            // both roots of z^2 + a1 z + a2 inside the unit circle (the Schur-Cohn / Jury conditions)
            if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
                return fail(KWS_ERR_INVALID, "filter %d section %d is not stable (a = %g, %g, %g)", k, s, q[3], q[4], q[5]);
            c[5 * s + 0] = q[0] / q[3];
            c[5 * s + 1] = q[1] / q[3];
            c[5 * s + 2] = q[2] / q[3];
            c[5 * s + 3] = -a1;
            c[5 * s + 4] = -a2;
        }
        // sosfilt_zi: the state of every section under a unit step in steady state, scaled by the DC gain of the sections before it
        std::vector<double> zi(n);
        double scale = 1.0;
        for (int s = 0; s < S; ++s) {
            const double *cs = &c[5 * s];
            const double g = (cs[0] + cs[1] + cs[2]) / (1.0 - cs[3] - cs[4]);
            zi[2 * s] = scale * (g - cs[0]);
            zi[2 * s + 1] = scale * (cs[2] + cs[4] * g);
            scale *= g;
        }
        // A column by column, then A^(2^e) by repeated squaring
        std::vector<double> A((size_t)n * n), T((size_t)n * n);
        for (int q = 0; q < n; ++q) {
            std::vector<double> z(n, 0.0);
            z[q] = 1.0;
            host_step(c, S, z);
            for (int r = 0; r < n; ++r) A[(size_t)r * n + q] = z[r];
        }
        double *dst = &table[(size_t)k * kStride];
        for (int i = 0; i < 5 * S; ++i) dst[i] = c[i];
        for (int q = 0; q < n; ++q) dst[5 * S + q] = zi[q];
        for (int e = 0; e < kPowers; ++e) {
            for (int i = 0; i < n * n; ++i) dst[kCoef + e * kMat + i] = A[i];
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < n; ++q) {
                    double acc = 0.0;
                    for (int j = 0; j < n; ++j) acc += A[(size_t)r * n + j] * A[(size_t)j * n + q];
                    T[(size_t)r * n + q] = acc;
                }
            A.swap(T);
        }
    }
    auto *fb = new kws_filter_bank();
    fb->K = K;
    fb->S = S;
    fb->padlen.assign(padlen, padlen + K);
    auto cleanup = [&](int rc) {
        kws_filter_bank_destroy(fb);
        return rc;
    };
    if (hipMalloc(&fb->table, sizeof(double) * table.size()) != hipSuccess || hipMalloc(&fb->d_padlen, sizeof(int32_t) * K) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "filter bank: device allocation for %d filters failed", K));
    }
    if (hipMemcpy(fb->table, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(fb->d_padlen, padlen, sizeof(int32_t) * K, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "filter bank: upload failed"));
    }
    *out = fb;
    return KWS_OK;
}

void kws_filter_bank_destroy(kws_filter_bank *fb)
{
    if (!fb) return;
    if (fb->table) (void)hipFree(fb->table);
    if (fb->d_padlen) (void)hipFree(fb->d_padlen);
    delete fb;
}

int kws_filter_bank_info(const kws_filter_bank *fb, int *K, int *n_sections, int32_t *padlen)
{
    if (!fb) return fail(KWS_ERR_INVALID, "null argument");
    if (K) *K = fb->K;
    if (n_sections) *n_sections = fb->S;
    if (padlen)
        for (int k = 0; k < fb->K; ++k) padlen[k] = fb->padlen[k];
    return KWS_OK;
}

int kws_filter_apply(const kws_filter_bank *fb, const kws_filter_params *p, const void *wav, int wav_dtype, const int32_t *index, int B,
                     int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const int32_t *explicit_filter, float *out,
                     int64_t out_stride, int32_t *lengths, int32_t *filter_used, void *stream)
{
    if (!fb || !p || (B > 0 && (!wav || !out || !lengths))) return fail(KWS_ERR_INVALID, "null argument");
    if (fb->K < 1) return fail(KWS_ERR_INVALID, "empty filter bank");
    if (!(p->filter_rate >= 0.f && p->filter_rate <= 1.f)) return fail(KWS_ERR_INVALID, "filter_rate %g is outside [0, 1]", (double)p->filter_rate);
    if (int rc = check_clip_batch(p->max_samples, KWS_FILTER_MAX_SAMPLES, B, stride, false, valid_len, position_base, &out_stride, wav_dtype))
        return rc;
    if (B > 0 && (const void *)out == wav && (wav_dtype != KWS_WAV_F32 || index || out_stride != stride))
        return fail(KWS_ERR_INVALID, "in place (out == wav) needs float32 input, no index and out_stride == stride");
    if (explicit_filter) {
        if (!filter_used && B > 0) return fail(KWS_ERR_INVALID, "explicit_filter needs filter_used (the choices are staged there)");
        for (int b = 0; b < B; ++b)
            if (explicit_filter[b] < -1 || explicit_filter[b] >= fb->K)
                return fail(KWS_ERR_INVALID, "clip %d: filter %d is outside [-1, %d)", b, explicit_filter[b], fb->K);
    }
    if (B == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (explicit_filter) KWS_HIP_CHECK(hipMemcpyAsync(filter_used, explicit_filter, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    const int ex = explicit_filter ? 1 : 0;
    switch (fb->S) {
    case 1: return launch<1>(fb, p, wav, wav_dtype, index, B, stride, valid_len, position_base, step, ex, out, out_stride, lengths, filter_used, s);
    case 2: return launch<2>(fb, p, wav, wav_dtype, index, B, stride, valid_len, position_base, step, ex, out, out_stride, lengths, filter_used, s);
    case 3: return launch<3>(fb, p, wav, wav_dtype, index, B, stride, valid_len, position_base, step, ex, out, out_stride, lengths, filter_used, s);
    default: return launch<4>(fb, p, wav, wav_dtype, index, B, stride, valid_len, position_base, step, ex, out, out_stride, lengths, filter_used, s);
    }
}

}  // extern "C"
