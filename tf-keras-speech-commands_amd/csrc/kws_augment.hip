// csrc/kws_augment.hip -- noise bank, plan kernel and apply kernel of the background-noise augmentation (include/kws.h; the mix of
// tools/audio_process/add_noise.py:19-35 of the reference).  The fused featurizer path lives with the featurizer (kws_featurize.hip).
#include <cfloat>
#include <cmath>
#include <vector>

#include "kws_common.h"
#include "kws_augment.h"
#include "kws_device.h"

namespace kws {

// One wave per clip: draw (or take) the record, then the gain.  p_v: fp32 lane partials over the voice head, an fp64 wave sum; p_n from
// the bank's prefix sums.  Lane 0 writes the record.
template <typename WavT>
__global__ __launch_bounds__(256) void augment_plan_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                           const int32_t *__restrict__ valid_len, int B, kws_augment_params p, int K,
                                                           const int32_t *__restrict__ seg_len, const double *__restrict__ prefix,
                                                           const int64_t *__restrict__ seg_start, int64_t position_base, uint32_t step,
                                                           int explicit_plan, kws_aug_clip *__restrict__ plan)
{
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= B) return;
    const ClipSrc src = clip_src(index, valid_len, stride, p.max_samples, b);
    const int lv = src.clipped;

    kws_aug_clip r;
    if (explicit_plan) {
        r = plan[b];
    } else {
        const uint32_t pos = aug_pos(position_base, b, kAugFields);
        r.apply = aug_unit(aug_hash(p.seed, step, pos + kAugApply)) < p.noised_rate ? 1 : 0;
        r.segment = (int)aug_uniform(aug_hash(p.seed, step, pos + kAugSegment), (uint32_t)K);
        r.snr_db = p.snr_db[aug_uniform(aug_hash(p.seed, step, pos + kAugSnr), (uint32_t)p.n_snr)];
        const int Lk = lv < seg_len[r.segment] ? lv : seg_len[r.segment];
        r.offset = r.apply ? (int)aug_uniform(aug_hash(p.seed, step, pos + kAugOffset), (uint32_t)(seg_len[r.segment] - Lk + 1)) : 0;
        r.shift = (int)aug_uniform(aug_hash(p.seed, step, pos + kAugShift), (uint32_t)(2 * p.max_shift + 1)) - p.max_shift;
    }
    const int k = r.segment;
    const int L = r.apply ? (lv < seg_len[k] ? lv : seg_len[k]) : lv;
    if (r.apply && r.offset > seg_len[k] - L) r.offset = seg_len[k] - L;
    float g = 0.f;
    if (r.apply && L > 0) {
        const WavT *v = wav + (int64_t)src.row * stride;
        float part = 0.f;
        for (int t = lane; t < L; t += 64) {
            const float x = aug_to_f32(v[t]);
            part = fmaf(x, x, part);
        }
        const double sv = wave_sum((double)part);
        const int64_t w0 = seg_start[k] + r.offset;
        const double pv = sv / L, pn = (prefix[w0 + L] - prefix[w0]) / L;
        g = (float)sqrt(pv / pow(10.0, (double)r.snr_db / 10.0) / (pn + (double)FLT_EPSILON));
    }
    r.apply = r.apply ? 1 : 0;
    r.length = L;
    r.gain = g;
    r.voice_length = lv;
    if (lane == 0) plan[b] = r;
}

template <typename WavT>
__global__ __launch_bounds__(256) void augment_apply_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                            const kws_aug_clip *__restrict__ plan, const float *__restrict__ bank,
                                                            const int64_t *__restrict__ seg_start, int max_samples, float *__restrict__ out,
                                                            int64_t out_stride, int32_t *__restrict__ lengths)
{
    const int b = blockIdx.x;                            // one block per clip
    const kws_aug_clip r = plan[b];
    const int row = index ? index[b] : b;
    const WavT *v = wav + (int64_t)row * stride;
    const float *n = bank + (r.apply ? seg_start[r.segment] + r.offset : 0);
    float *dst = out + (int64_t)b * out_stride;
    // to out_stride, as every sibling stage: aug_sample is 0 from r.length (<= max_samples) on
    for (int64_t t = (int64_t)threadIdx.x; t < out_stride; t += (int64_t)blockDim.x)
        dst[t] = t < max_samples ? aug_sample(v, n, r.length, r.shift, r.gain, r.apply != 0, (int)t) : 0.f;
    if (lengths && threadIdx.x == 0) lengths[b] = r.length;
}

int augment_apply_launch(const kws_noise_bank *bank, const kws_aug_clip *plan, const void *wav, int wav_dtype, const int32_t *index, int B,
                         int64_t stride, int max_samples, float *out, int64_t out_stride, int32_t *lengths, hipStream_t s)
{
    if (B == 0 || max_samples == 0) return KWS_OK;
    const dim3 grid((unsigned)B), block(256);
    return for_wav_type(wav_dtype, "augment_apply_f32", "augment_apply_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        KWS_LAUNCH(name, augment_apply_kernel<WavT>, grid, block, 0, s, static_cast<const WavT *>(wav), stride, index, plan, bank->samples,
                   bank->d_start, max_samples, out, out_stride, lengths);
        KWS_LAUNCH_CHECK("augment_apply_kernel");
        return KWS_OK;
    });
}

}  // namespace kws

using namespace kws;

extern "C" {

int kws_noise_bank_create(const void *samples, int wav_dtype, const int32_t *seg_len, int K, kws_noise_bank **out)
{
    if (!out || !seg_len || !samples) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (K < 1) return fail(KWS_ERR_INVALID, "a noise bank needs at least one segment");
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    auto *nb = new kws_noise_bank();
    nb->K = K;
    nb->start.resize(K);
    nb->len.assign(seg_len, seg_len + K);
    for (int k = 0; k < K; ++k) {
        if (seg_len[k] < 1) { delete nb; return fail(KWS_ERR_INVALID, "noise segment %d is empty", k); }
        nb->start[k] = nb->total;
        nb->total += seg_len[k];
    }
    std::vector<float> x((size_t)nb->total);
    std::vector<double> pre((size_t)nb->total + 1);
    pre[0] = 0.0;
    for (int64_t i = 0; i < nb->total; ++i) {
        x[i] = wav_dtype == KWS_WAV_F32 ? static_cast<const float *>(samples)[i] : (float)static_cast<const short *>(samples)[i] * (1.0f / 32768.0f);
        pre[i + 1] = pre[i] + (double)x[i] * (double)x[i];
    }
    auto cleanup = [&](int rc) {
        kws_noise_bank_destroy(nb);
        return rc;
    };
    if (hipMalloc(&nb->samples, sizeof(float) * nb->total) != hipSuccess || hipMalloc(&nb->prefix, sizeof(double) * (nb->total + 1)) != hipSuccess ||
        hipMalloc(&nb->d_start, sizeof(int64_t) * K) != hipSuccess || hipMalloc(&nb->d_len, sizeof(int32_t) * K) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "noise bank: device allocation of %lld samples failed", (long long)nb->total));
    }
    if (hipMemcpy(nb->samples, x.data(), sizeof(float) * nb->total, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(nb->prefix, pre.data(), sizeof(double) * (nb->total + 1), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(nb->d_start, nb->start.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(nb->d_len, nb->len.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "noise bank: upload failed"));
    }
    *out = nb;
    return KWS_OK;
}

void kws_noise_bank_destroy(kws_noise_bank *nb)
{
    if (!nb) return;
    if (nb->samples) (void)hipFree(nb->samples);
    if (nb->prefix) (void)hipFree(nb->prefix);
    if (nb->d_start) (void)hipFree(nb->d_start);
    if (nb->d_len) (void)hipFree(nb->d_len);
    delete nb;
}

int kws_noise_bank_info(const kws_noise_bank *nb, int *K, int64_t *total, int32_t *seg_len)
{
    if (!nb) return fail(KWS_ERR_INVALID, "null argument");
    if (K) *K = nb->K;
    if (total) *total = nb->total;
    if (seg_len) std::copy(nb->len.begin(), nb->len.end(), seg_len);
    return KWS_OK;
}

// The SNRs the plan accepts (include/kws.h): at +-200 dB and |v| <= 1 the gain sqrt(p_v / 10^(s/10) / FLT_EPSILON) is at most 2.9e13,
// finite in float32 with 25 orders of magnitude to spare; from -702 dB on it is inf.  NaN fails both comparisons.
constexpr float kMaxSnrDb = 200.f;
static bool snr_ok(float s) { return s >= -kMaxSnrDb && s <= kMaxSnrDb; }

static int check_params(const kws_augment_params *p)
{
    if (!p) return fail(KWS_ERR_INVALID, "null augment params");
    if (!(p->noised_rate >= 0.f && p->noised_rate <= 1.f)) return fail(KWS_ERR_INVALID, "noised_rate %g is outside [0, 1]", (double)p->noised_rate);
    if (p->n_snr < 1 || p->n_snr > KWS_AUG_MAX_SNR) return fail(KWS_ERR_INVALID, "the SNR list needs 1..%d entries, got %d", KWS_AUG_MAX_SNR, p->n_snr);
    for (int i = 0; i < p->n_snr; ++i)
        if (!snr_ok(p->snr_db[i]))
            return fail(KWS_ERR_INVALID, "SNR %d (%g dB) is outside [%g, %g]", i, (double)p->snr_db[i], -(double)kMaxSnrDb, (double)kMaxSnrDb);
    if (p->max_shift < 0) return fail(KWS_ERR_INVALID, "max_shift %d is negative", p->max_shift);
    if (p->max_shift > (1 << 24)) return fail(KWS_ERR_INVALID, "max_shift %d is too large", p->max_shift);
    return KWS_OK;
}

int kws_augment_plan(const kws_noise_bank *bank, const kws_augment_params *params, const void *wav, int wav_dtype, const int32_t *index,
                     int B, int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, kws_aug_clip *plan,
                     const kws_aug_clip *explicit_plan, void *stream)
{
    // what needs no bank comes first, so that a caller's values are judged the same with and without a device
    if (!plan || (!wav && B > 0)) return fail(KWS_ERR_INVALID, "null argument");
    if (int rc = check_params(params)) return rc;
    if (int rc = check_clip_batch(params->max_samples, INT_MAX, B, stride, false, valid_len, position_base, nullptr, wav_dtype)) return rc;
    if (explicit_plan)
        for (int b = 0; b < B; ++b) {
            const kws_aug_clip &r = explicit_plan[b];
            if (!snr_ok(r.snr_db))
                return fail(KWS_ERR_INVALID, "clip %d: SNR %g dB is outside [%g, %g]", b, (double)r.snr_db, -(double)kMaxSnrDb, (double)kMaxSnrDb);
            if (r.shift < -(1 << 24) || r.shift > (1 << 24)) return fail(KWS_ERR_INVALID, "clip %d: shift %d is too large", b, r.shift);
        }
    if (!bank) return fail(KWS_ERR_INVALID, "null noise bank");
    if (bank->K < 1) return fail(KWS_ERR_INVALID, "empty noise bank");
    if (explicit_plan)
        for (int b = 0; b < B; ++b) {
            const kws_aug_clip &r = explicit_plan[b];
            if (r.segment < 0 || r.segment >= bank->K) return fail(KWS_ERR_INVALID, "clip %d: segment %d is outside [0, %d)", b, r.segment, bank->K);
            if (r.offset < 0 || r.offset >= bank->len[r.segment])
                return fail(KWS_ERR_INVALID, "clip %d: offset %d is outside segment %d (%d samples)", b, r.offset, r.segment, bank->len[r.segment]);
        }
    if (B == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (explicit_plan) KWS_HIP_CHECK(hipMemcpyAsync(plan, explicit_plan, sizeof(kws_aug_clip) * B, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    return for_wav_type(wav_dtype, "augment_plan_f32", "augment_plan_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        KWS_LAUNCH(name, augment_plan_kernel<WavT>, grid, block, 0, s, static_cast<const WavT *>(wav), stride, index, valid_len, B, *params,
                   bank->K, bank->d_len, bank->prefix, bank->d_start, position_base, (uint32_t)step, explicit_plan ? 1 : 0, plan);
        KWS_LAUNCH_CHECK("augment_plan_kernel");
        return KWS_OK;
    });
}

int kws_augment_apply(const kws_noise_bank *bank, const kws_aug_clip *plan, const void *wav, int wav_dtype, const int32_t *index, int B,
                      int64_t stride, int max_samples, float *out, int64_t out_stride, int32_t *lengths, void *stream)
{
    if (!bank || !out || (B > 0 && (!plan || !wav))) return fail(KWS_ERR_INVALID, "null argument");
    if (bank->K < 1) return fail(KWS_ERR_INVALID, "empty noise bank");
    if (B < 0 || stride < 0 || max_samples < 0) return fail(KWS_ERR_INVALID, "negative batch, stride or max_samples");
    if (out_stride < max_samples) return fail(KWS_ERR_INVALID, "out_stride %lld < max_samples %d", (long long)out_stride, max_samples);
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    return augment_apply_launch(bank, plan, wav, wav_dtype, index, B, stride, max_samples, out, out_stride, lengths, static_cast<hipStream_t>(stream));
}

}  // extern "C"
