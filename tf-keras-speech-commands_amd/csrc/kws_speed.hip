// csrc/kws_speed.hip -- interpolation table and the apply kernel of the speed and loudness perturbation (include/kws.h: kws_resampler_*,
// kws_speed_apply; the resampling and the --loudness gain of tools/audio_process/audio_convert.py of the reference).
//
// One 256-thread block per clip.  A resampled clip's block copies the table (Z P + 1 floats, 32 KiB at the default geometry) into LDS;
// thread i then makes the outputs n = i, i + 256, ...: neighbouring outputs read overlapping source windows, so a wave's source loads
// fall into a few cache lines and the source stays in global memory.  The phase arithmetic (t = n r, pos = ((phi + k) s) P, its floor
// and its fraction; kws_resample.h, shared with kws_pitch.hip) is fp64 with contraction off, so that the table index and the last tap of a wing are the ones the float64
// restatement of the tests takes; weights, products and sums are fp32 in a fixed order (left wing, right wing, k ascending).
// The level needs the mean square of the whole output before it can scale: every thread sums the squares of its own outputs in fp64,
// the block adds them in a fixed order (butterfly within a wave, waves in order), and every thread then scales the outputs it wrote
// itself (they come back from L2; a clip that is not resampled is read from the source a second time and written once).  No atomics.
#include <cfloat>
#include <climits>
#include <cmath>

#include "kws_common.h"
#include "kws_wave_stage.h"
#include "kws_device.h"
#include "kws_resample.h"

namespace kws {
namespace spd {

constexpr int kThreads = 256, kWaves = kThreads / 64;
enum { kSpdApply = 0, kSpdRatio = 1, kSpdLevel = 2, kSpdTarget = 3, kSpdFields = 4 };   // draw fields: aug_hash(seed_s, step, 4 p + f)

template <typename WavT>
__global__ __launch_bounds__(kThreads) void speed_apply_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                               const int32_t *__restrict__ valid_len, kws_speed_params p,
                                                               const float *__restrict__ table, int Z, int P, int64_t position_base,
                                                               uint32_t step, int explicit_speed, int explicit_db, float *__restrict__ out,
                                                               int64_t out_stride, int32_t *__restrict__ lengths, float *speed_used,
                                                               float *gain_used)
{
    extern __shared__ float h[];                             // the table, when this clip is resampled
    __shared__ double part[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ms = p.max_samples;
    const ClipSrc src = clip_src(index, valid_len, stride, ms, b);
    const int Ls = src.len;                                  // the whole valid length is the source of a resampled clip

    const uint32_t pos0 = aug_pos(position_base, b, kSpdFields);
    float r = 0.f, target = 0.f;
    bool levelled;
    if (explicit_speed) r = speed_used[b];                   // the host's values, staged in the outputs by kws_speed_apply
    else if (aug_unit(aug_hash(p.seed, step, pos0 + kSpdApply)) < p.speed_rate)
        r = __fmaf_rn(aug_unit(aug_hash(p.seed, step, pos0 + kSpdRatio)), p.speed_hi - p.speed_lo, p.speed_lo);
    if (explicit_db) {
        target = gain_used[b];
        levelled = !(target != target);
    } else {
        levelled = aug_unit(aug_hash(p.seed, step, pos0 + kSpdLevel)) < p.loud_rate;
        target = __fmaf_rn(aug_unit(aug_hash(p.seed, step, pos0 + kSpdTarget)), p.loud_hi_db - p.loud_lo_db, p.loud_lo_db);
    }
    const bool resampled = r != 0.f;
    const double rd = (double)r;
    int lo = src.clipped;
    if (resampled && Ls > 0) {
        const double q = ceil((double)Ls / rd);
        lo = q < (double)ms ? (int)q : ms;
    }
    __syncthreads();                                         // every thread has read the staged values before thread 0 overwrites them
    if (tid == 0) {
        lengths[b] = lo;
        if (speed_used) speed_used[b] = r;
        if (gain_used && !levelled) gain_used[b] = 1.f;
    }
    const WavT *v = wav + (int64_t)src.row * stride;
    float *dst = out + (int64_t)b * out_stride;
    if (!resampled && !levelled) {                           // left as it is: the f32 conversion
        dry_copy<kThreads>(dst, v, lo, out_stride);
        return;
    }
    double sq = 0.0;
    if (resampled) {
        const int n_table = Z * P + 1;
        for (int i = tid; i < n_table; i += kThreads) h[i] = table[i];
        __syncthreads();
        const double s = rd > 1.0 ? 1.0 / rd : 1.0, dP = (double)P, lim = (double)(Z * P);
        const float sf = (float)s;
        for (int n = tid; n < lo; n += kThreads) {
            const float y = resample_at(v, h, n, Ls, rd, s, sf, dP, lim);
            dst[n] = y;
            sq += (double)y * (double)y;
        }
    } else {
        for (int n = tid; n < lo; n += kThreads) {
            const float y = aug_to_f32(v[n]);
            sq += (double)y * (double)y;
        }
    }
    if (levelled) {
        sq = wave_sum(sq);
        if ((tid & 63) == 0) part[tid >> 6] = sq;
        __syncthreads();
        double total = part[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) total += part[w];
        const double m = lo > 0 ? total / (double)lo : 0.0;
        const float g = sqrtf((float)(pow(10.0, (double)target / 10.0) / (m + (double)FLT_EPSILON)));
        if (tid == 0 && gain_used) gain_used[b] = g;
        if (resampled)
            for (int n = tid; n < lo; n += kThreads) dst[n] *= g;          // this thread's own stores
        else
            for (int n = tid; n < lo; n += kThreads) dst[n] = aug_to_f32(v[n]) * g;
    }
    for (int64_t t = (int64_t)lo + tid; t < out_stride; t += kThreads) dst[t] = 0.f;
}

// I0 by its power series (every term positive: no cancellation), float64
double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// the table's copy on the current device
int device_table(const kws_resampler *rs, const float **out)
{
    kws_resampler *m = const_cast<kws_resampler *>(rs);
    int dev = 0;
    KWS_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(m->mu);
    float *&d = m->dev[dev];
    if (!d) {
        const size_t bytes = sizeof(float) * m->table.size();
        if (hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
            return fail(KWS_ERR_HIP, "resampler: device allocation of %zu bytes failed", bytes);
        }
        if (hipMemcpy(d, m->table.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d);
            d = nullptr;
            return fail(KWS_ERR_HIP, "resampler: upload failed");
        }
    }
    *out = d;
    return KWS_OK;
}

}  // namespace spd
}  // namespace kws

using namespace kws;
using namespace kws::spd;

extern "C" {

int kws_resampler_create(int zero_crossings, int phases, double beta, double rolloff, kws_resampler **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (zero_crossings < 4 || zero_crossings > 32) return fail(KWS_ERR_INVALID, "zero_crossings %d is outside [4, 32]", zero_crossings);
    if (phases < 32 || phases > 1024) return fail(KWS_ERR_INVALID, "phases %d is outside [32, 1024]", phases);
    if (!(beta >= 0.0 && beta <= 20.0)) return fail(KWS_ERR_INVALID, "beta %g is outside [0, 20]", beta);
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(KWS_ERR_INVALID, "rolloff %g is outside (0, 1]", rolloff);
    const size_t n = (size_t)zero_crossings * (size_t)phases + 1;
    if (n * sizeof(float) > kMaxTableBytes)
        return fail(KWS_ERR_UNSUPPORTED, "a table of %d x %d + 1 floats does not fit %zu bytes of LDS", zero_crossings, phases, kMaxTableBytes);
    auto *rs = new kws_resampler();
    rs->Z = zero_crossings;
    rs->P = phases;
    rs->beta = beta;
    rs->rolloff = rolloff;
    rs->table.resize(n);
    const double pi = 3.14159265358979323846, i0b = bessel_i0(beta);
    for (size_t i = 0; i < n; ++i) {
        const double x = rolloff * (double)i / (double)phases, u = (double)i / ((double)phases * (double)zero_crossings);
        const double sinc = i == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double a = 1.0 - u * u;
        rs->table[i] = (float)(rolloff * sinc * bessel_i0(beta * std::sqrt(a > 0.0 ? a : 0.0)) / i0b);
    }
    *out = rs;
    return KWS_OK;
}

void kws_resampler_destroy(kws_resampler *rs)
{
    if (!rs) return;
    for (auto &kv : rs->dev)
        if (kv.second) (void)hipFree(kv.second);
    delete rs;
}

int kws_resampler_info(const kws_resampler *rs, int *zero_crossings, int *phases, double *beta, double *rolloff)
{
    if (!rs) return fail(KWS_ERR_INVALID, "null argument");
    if (zero_crossings) *zero_crossings = rs->Z;
    if (phases) *phases = rs->P;
    if (beta) *beta = rs->beta;
    if (rolloff) *rolloff = rs->rolloff;
    return KWS_OK;
}

int kws_resampler_table(const kws_resampler *rs, float *out, size_t n)
{
    if (!rs || !out) return fail(KWS_ERR_INVALID, "null argument");
    if (n < rs->table.size()) return fail(KWS_ERR_INVALID, "the table has %zu floats, room for %zu", rs->table.size(), n);
    for (size_t i = 0; i < rs->table.size(); ++i) out[i] = rs->table[i];
    return KWS_OK;
}

int kws_speed_apply(const kws_resampler *rs, const kws_speed_params *p, const void *wav, int wav_dtype, const int32_t *index, int B,
                    int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const float *explicit_speed,
                    const float *explicit_db, float *out, int64_t out_stride, int32_t *lengths, float *speed_used, float *gain_used,
                    void *stream)
{
    if (!p || (B > 0 && (!wav || !out || !lengths))) return fail(KWS_ERR_INVALID, "null argument");
    if (!(p->speed_rate >= 0.f && p->speed_rate <= 1.f)) return fail(KWS_ERR_INVALID, "speed_rate %g is outside [0, 1]", (double)p->speed_rate);
    if (!(p->loud_rate >= 0.f && p->loud_rate <= 1.f)) return fail(KWS_ERR_INVALID, "loud_rate %g is outside [0, 1]", (double)p->loud_rate);
    if (p->speed_rate > 0.f && !(0.5f <= p->speed_lo && p->speed_lo <= p->speed_hi && p->speed_hi <= 2.f))
        return fail(KWS_ERR_INVALID, "speed range [%g, %g] needs 0.5 <= lo <= hi <= 2", (double)p->speed_lo, (double)p->speed_hi);
    if (p->loud_rate > 0.f && !(-80.f <= p->loud_lo_db && p->loud_lo_db <= p->loud_hi_db && p->loud_hi_db <= 0.f))
        return fail(KWS_ERR_INVALID, "loudness range [%g, %g] dBFS needs -80 <= lo <= hi <= 0", (double)p->loud_lo_db, (double)p->loud_hi_db);
    if (int rc = check_clip_batch(p->max_samples, INT_MAX, B, stride, true, valid_len, position_base, &out_stride, wav_dtype)) return rc;
    if (B > 0 && (const void *)out == wav) return fail(KWS_ERR_INVALID, "the perturbation cannot run in place (out == wav)");
    bool needs_table = !explicit_speed && p->speed_rate > 0.f;
    if (explicit_speed) {
        if (!speed_used && B > 0) return fail(KWS_ERR_INVALID, "explicit_speed needs speed_used (the ratios are staged there)");
        for (int b = 0; b < B; ++b) {
            if (explicit_speed[b] != 0.f && !(explicit_speed[b] >= 0.5f && explicit_speed[b] <= 2.f))
                return fail(KWS_ERR_INVALID, "clip %d: ratio %g is neither 0 nor in [0.5, 2]", b, (double)explicit_speed[b]);
            needs_table = needs_table || explicit_speed[b] != 0.f;
        }
    }
    if (!rs && needs_table) return fail(KWS_ERR_INVALID, "a speed change needs a resampler (the interpolation table)");
    if (explicit_db) {
        if (!gain_used && B > 0) return fail(KWS_ERR_INVALID, "explicit_db needs gain_used (the targets are staged there)");
        for (int b = 0; b < B; ++b)
            if (!std::isnan(explicit_db[b]) && !(explicit_db[b] >= -80.f && explicit_db[b] <= 0.f))
                return fail(KWS_ERR_INVALID, "clip %d: target %g dBFS is neither NaN nor in [-80, 0]", b, (double)explicit_db[b]);
    }
    if (B == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *table = nullptr;
    size_t lds = 0;
    if (rs) {
        const int rc = device_table(rs, &table);
        if (rc != KWS_OK) return rc;
        lds = sizeof(float) * rs->table.size();
    }
    if (explicit_speed) KWS_HIP_CHECK(hipMemcpyAsync(speed_used, explicit_speed, sizeof(float) * B, hipMemcpyHostToDevice, s));
    if (explicit_db) KWS_HIP_CHECK(hipMemcpyAsync(gain_used, explicit_db, sizeof(float) * B, hipMemcpyHostToDevice, s));
    const int Z = rs ? rs->Z : 0, P = rs ? rs->P : 0, exs = explicit_speed ? 1 : 0, exd = explicit_db ? 1 : 0;
    const dim3 grid((unsigned)B), block(kThreads);
    return for_wav_type(wav_dtype, "speed_apply_f32", "speed_apply_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        if (lds)
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&speed_apply_kernel<WavT>), (int)lds)) return rc;
        KWS_LAUNCH(name, (speed_apply_kernel<WavT>), grid, block, lds, s, static_cast<const WavT *>(wav), stride, index, valid_len, *p, table,
                   Z, P, position_base, (uint32_t)step, exs, exd, out, out_stride, lengths, speed_used, gain_used);
        KWS_LAUNCH_CHECK("speed_apply_kernel");
        return KWS_OK;
    });
}

}  // extern "C"
