// csrc/kws_specaug.hip -- SpecAugment of the features: time warp, time masks and frequency masks (include/kws.h: kws_feature_mask_draw,
// kws_feature_mask, kws_feature_mask_max_clip).  The stage sits behind the featurizer (or the gather of cached features) and in front of
// the model; include/kws.h defines the transformation, tests/specaug_ref.py restates it in numpy.
//
// One wave per clip, four waves per 256-thread block; the waves of a block share nothing, so there is no block barrier and a wave
// whose clip is not applied leaves at once (in place it moves no bytes; out of place it copies global to global).  An applied clip is
// loaded once into the wave's slice of the LDS -- after that the wave reads no global memory, which is what makes out == feat safe for
// the warp, whose output frame t reads the input frames k and k + 1 on either side of it.  Then:
//   mean (KWS_FMASK_MEAN with a mask of positive width): lanes own coefficients; lane f sums the warped column y[.][f] in ascending t
//         out of the LDS (neighbouring lanes read neighbouring banks) and parks sum / T behind the clip;
//   store: lanes own elements, four consecutive ones where the clip size and both bases allow 16-byte accesses, one otherwise; an
//         element is the fill value inside a mask, the warp's interpolation of two LDS values outside (the clip itself without warp).
// The warp's source position is recomputed per element from the wave-uniform (c, d): the same float32 operations in the mean and in the
// store, so both see the same y.  No atomics, no cross-wave communication, fixed summation order.
#include "kws_common.h"
#include "kws_wave_stage.h"

namespace kws {
namespace fmask {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFields = 32;                                       // draw fields per clip: aug_hash(seed_m, step, 32 p + f)
enum { kApply = 0, kWarpCenter = 1, kWarpShift = 2, kTime = 3, kFreq = 11 };
// a wave's slice of the 160 KiB a block may have: the clip (rounded up to 16 bytes) and its F fill values, and F <= T F
constexpr int kWaveFloats = 160 * 1024 / (int)sizeof(float) / kWaves;
constexpr int kMaxClip = kWaveFloats / 2;
static_assert(kMaxClip >= 124 * 40 && kMaxClip % 4 == 0, "the slice must hold a 124 x 40 clip and stay 16-byte aligned");

// the plan of the clip at global position `position` (every field, whether or not the clip is applied); p was checked by check_params
__host__ __device__ inline void draw_clip(const kws_feature_mask_params &p, int T, int F, int64_t position, uint32_t step, kws_fmask_clip &c)
{
    const uint32_t pos = (uint32_t)position * (uint32_t)kFields;
    c.apply = aug_unit(aug_hash(p.seed, step, pos + kApply)) < p.rate ? 1 : 0;
    const int W = p.max_warp;
    c.warp_center = c.warp_shift = 0;
    if (W > 0) {
        c.warp_center = W + 1 + (int)aug_uniform(aug_hash(p.seed, step, pos + kWarpCenter), (uint32_t)(T - 2 * W - 2));
        c.warp_shift = (int)aug_uniform(aug_hash(p.seed, step, pos + kWarpShift), (uint32_t)(2 * W + 1)) - W;
    }
    c.n_time = p.n_time;
    c.n_freq = p.n_freq;
#pragma unroll
    for (int i = 0; i < KWS_FMASK_MAX; ++i) {
        c.t0[i] = c.tw[i] = c.f0[i] = c.fw[i] = 0;
        if (i < p.n_time) {
            c.tw[i] = (int)aug_uniform(aug_hash(p.seed, step, pos + kTime + 2 * i), (uint32_t)(p.max_time_width + 1));
            c.t0[i] = (int)aug_uniform(aug_hash(p.seed, step, pos + kTime + 1 + 2 * i), (uint32_t)(T - c.tw[i] + 1));
        }
        if (i < p.n_freq) {
            c.fw[i] = (int)aug_uniform(aug_hash(p.seed, step, pos + kFreq + 2 * i), (uint32_t)(p.max_freq_width + 1));
            c.f0[i] = (int)aug_uniform(aug_hash(p.seed, step, pos + kFreq + 1 + 2 * i), (uint32_t)(F - c.fw[i] + 1));
        }
    }
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave-uniform half of a clip's plan as the passes use it.
struct Warp {
    int on, c, cd, T;            // cd = c + d
};

// y[t][f] of the clip in the LDS slice x (row length F)
__device__ __forceinline__ float warped(const float *x, const Warp &w, int t, int f, int F)
{
#pragma clang fp contract(off)
    if (!w.on) return x[t * F + f];
    float s;
    if (t <= w.cd) s = __fdiv_rn((float)(t * w.c), (float)w.cd);
    else s = (float)w.c + __fdiv_rn((float)((t - w.cd) * (w.T - 1 - w.c)), (float)(w.T - 1 - w.cd));
    int k = (int)s;
    k = k > w.T - 2 ? w.T - 2 : k < 0 ? 0 : k;               // k < 0 cannot happen for a checked plan: the LDS index stays inside the clip
    const float fr = s - (float)k;
    const float a = x[k * F + f], b = x[(k + 1) * F + f];
    if (fr == 0.f) return a;
    if (fr == 1.f) return b;
    return (1.f - fr) * a + fr * b;
}

__device__ __forceinline__ bool covered(const int32_t *start, const int32_t *width, int n, int v)
{
    bool m = false;
#pragma unroll
    for (int i = 0; i < KWS_FMASK_MAX; ++i) m = m || (i < n && v >= start[i] && v < start[i] + width[i]);
    return m;
}

// kVec: T F is a multiple of 4 and feat and out are 16-byte aligned, so every clip starts on a 16-byte boundary
template <bool kVec>
__global__ __launch_bounds__(kThreads) void feature_mask_kernel(const float *feat, float *out, int B, int T, int F, int slice,
                                                                kws_feature_mask_params p, int64_t position_base, uint32_t step,
                                                                int explicit_plan, kws_fmask_clip *plan)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = (int)blockIdx.x * kWaves + wave;
    if (b >= B) return;                                      // the waves of a block share nothing: no barrier follows
    kws_fmask_clip c;
    if (explicit_plan) c = plan[b];                          // the host's records, staged in plan_out by kws_feature_mask
    else {
        draw_clip(p, T, F, position_base + b, step, c);
        if (plan && lane == 0) plan[b] = c;
    }
    const int n = T * F;
    const float *src = feat + (int64_t)b * n;
    float *dst = out + (int64_t)b * n;
    if (!c.apply) {
        if (src == dst) return;
        if (kVec) {
            for (int i = lane; i < n / 4; i += 64) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
        } else {
            for (int i = lane; i < n; i += 64) dst[i] = src[i];
        }
        return;
    }
    float *x = lds + (size_t)wave * slice;
    float *mean = x + ((n + 3) & ~3);
    if (kVec) {
        for (int i = lane; i < n / 4; i += 64) reinterpret_cast<float4 *>(x)[i] = reinterpret_cast<const float4 *>(src)[i];
    } else {
        for (int i = lane; i < n; i += 64) x[i] = src[i];
    }
    wave_sync();                                             // the clip is in the LDS: from here on the wave reads no global memory

    Warp w;
    w.on = c.warp_center > 0 && T >= 3;
    w.c = c.warp_center;
    w.cd = c.warp_center + c.warp_shift;
    w.T = T;
    bool any = false;
#pragma unroll
    for (int i = 0; i < KWS_FMASK_MAX; ++i) any = any || (i < c.n_time && c.tw[i] > 0) || (i < c.n_freq && c.fw[i] > 0);
    const bool use_mean = p.fill == KWS_FMASK_MEAN && any;
    if (use_mean) {
        const float count = (float)T;
        for (int f = lane; f < F; f += 64) {
            float sum = 0.f;
            for (int t = 0; t < T; ++t) sum += warped(x, w, t, f, F);
            mean[f] = __fdiv_rn(sum, count);
        }
        wave_sync();
    }

    if (kVec) {
        for (int i = lane; i < n / 4; i += 64) {
            int t = (4 * i) / F, f = 4 * i - t * F;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool m = covered(c.t0, c.tw, c.n_time, t) || covered(c.f0, c.fw, c.n_freq, f);
                v[j] = m ? (use_mean ? mean[f] : 0.f) : warped(x, w, t, f, F);
                if (++f == F) {
                    f = 0;
                    ++t;
                }
            }
            reinterpret_cast<float4 *>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int i = lane; i < n; i += 64) {
            const int t = i / F, f = i - t * F;
            const bool m = covered(c.t0, c.tw, c.n_time, t) || covered(c.f0, c.fw, c.n_freq, f);
            dst[i] = m ? (use_mean ? mean[f] : 0.f) : warped(x, w, t, f, F);
        }
    }
}

// the parameter errors kws_feature_mask_draw and kws_feature_mask share
int check_params(const kws_feature_mask_params *p, int T, int F)
{
    if (!p) return fail(KWS_ERR_INVALID, "null argument");
    if (T < 1 || F < 1) return fail(KWS_ERR_INVALID, "a clip of %d x %d features", T, F);
    if (!(p->rate >= 0.f && p->rate <= 1.f)) return fail(KWS_ERR_INVALID, "rate %g is outside [0, 1]", (double)p->rate);
    if (p->n_time < 0 || p->n_time > KWS_FMASK_MAX) return fail(KWS_ERR_INVALID, "%d time masks are outside [0, %d]", p->n_time, KWS_FMASK_MAX);
    if (p->n_freq < 0 || p->n_freq > KWS_FMASK_MAX)
        return fail(KWS_ERR_INVALID, "%d frequency masks are outside [0, %d]", p->n_freq, KWS_FMASK_MAX);
    if (p->max_time_width < 0 || p->max_time_width > T) return fail(KWS_ERR_INVALID, "max_time_width %d is outside [0, %d]", p->max_time_width, T);
    if (p->max_freq_width < 0 || p->max_freq_width > F) return fail(KWS_ERR_INVALID, "max_freq_width %d is outside [0, %d]", p->max_freq_width, F);
    if (p->max_warp < 0) return fail(KWS_ERR_INVALID, "max_warp %d is negative", p->max_warp);
    if (p->max_warp > 0 && (int64_t)T < 2 * (int64_t)p->max_warp + 3)
        return fail(KWS_ERR_INVALID, "a time warp of up to %d frames needs at least %lld frames, got %d", p->max_warp,
                    2 * (long long)p->max_warp + 3, T);
    if (p->fill != KWS_FMASK_ZERO && p->fill != KWS_FMASK_MEAN) return fail(KWS_ERR_INVALID, "unknown fill %d", p->fill);
    return KWS_OK;
}

int check_masks(int b, const char *what, int n, const int32_t *start, const int32_t *width, int size)
{
    if (n < 0 || n > KWS_FMASK_MAX) return fail(KWS_ERR_INVALID, "clip %d: %d %s masks are outside [0, %d]", b, n, what, KWS_FMASK_MAX);
    for (int i = 0; i < n; ++i)
        if (start[i] < 0 || width[i] < 0 || (int64_t)start[i] + width[i] > size)
            return fail(KWS_ERR_INVALID, "clip %d: %s mask %d [%d, %d + %d) leaves [0, %d]", b, what, i, start[i], start[i], width[i], size);
    return KWS_OK;
}

}  // namespace fmask
}  // namespace kws

using namespace kws;
using namespace kws::fmask;

extern "C" {

int64_t kws_feature_mask_max_clip(void) { return kMaxClip; }

int kws_feature_mask_draw(const kws_feature_mask_params *p, int T, int F, int64_t position, int64_t step, kws_fmask_clip *out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    if (int rc = check_params(p, T, F)) return rc;
    if (position < 0) return fail(KWS_ERR_INVALID, "negative position");
    draw_clip(*p, T, F, position, (uint32_t)step, *out);
    return KWS_OK;
}

int kws_feature_mask(const kws_feature_mask_params *p, const float *feat, float *out, int B, int T, int F, int64_t position_base,
                     int64_t step, const kws_fmask_clip *explicit_plan, kws_fmask_clip *plan_out, void *stream)
{
    if (int rc = check_params(p, T, F)) return rc;
    if (B < 0 || position_base < 0) return fail(KWS_ERR_INVALID, "negative batch or position_base");
    if ((int64_t)T * F > kMaxClip)
        return fail(KWS_ERR_UNSUPPORTED, "a clip of %d x %d features is larger than %d (a wave's share of the LDS)", T, F, kMaxClip);
    if (B == 0) return KWS_OK;
    if (!feat || !out) return fail(KWS_ERR_INVALID, "null argument");
    if (explicit_plan) {
        if (!plan_out) return fail(KWS_ERR_INVALID, "explicit_plan needs plan_out (the records are staged there)");
        for (int b = 0; b < B; ++b) {
            const kws_fmask_clip &r = explicit_plan[b];
            if (r.apply != 0 && r.apply != 1) return fail(KWS_ERR_INVALID, "clip %d: apply %d is neither 0 nor 1", b, r.apply);
            if (int rc = check_masks(b, "time", r.n_time, r.t0, r.tw, T)) return rc;
            if (int rc = check_masks(b, "frequency", r.n_freq, r.f0, r.fw, F)) return rc;
            const int64_t cd = (int64_t)r.warp_center + r.warp_shift;
            if (!(r.warp_center == 0 && r.warp_shift == 0) && !(r.warp_center >= 1 && r.warp_center <= T - 2 && cd >= 1 && cd <= T - 2))
                return fail(KWS_ERR_INVALID, "clip %d: warp of frame %d by %d leaves [1, %d]", b, r.warp_center, r.warp_shift, T - 2);
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (explicit_plan) KWS_HIP_CHECK(hipMemcpyAsync(plan_out, explicit_plan, sizeof(kws_fmask_clip) * B, hipMemcpyHostToDevice, s));
    const int n = T * F;
    const int slice = ((n + 3) & ~3) + ((F + 3) & ~3);       // floats, a multiple of 16 bytes; <= kWaveFloats since F <= n <= kMaxClip
    const size_t lds = sizeof(float) * (size_t)slice * kWaves;
    const bool vec = n % 4 == 0 && ((uintptr_t)feat | (uintptr_t)out) % 16 == 0;
    const dim3 grid((unsigned)((B + kWaves - 1) / kWaves)), block(kThreads);
    const int ex = explicit_plan ? 1 : 0;
    if (vec) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&feature_mask_kernel<true>), (int)lds)) return rc;
        KWS_LAUNCH("feature_mask_vec", (feature_mask_kernel<true>), grid, block, lds, s, feat, out, B, T, F, slice, *p, position_base,
                   (uint32_t)step, ex, plan_out);
    } else {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&feature_mask_kernel<false>), (int)lds)) return rc;
        KWS_LAUNCH("feature_mask_scalar", (feature_mask_kernel<false>), grid, block, lds, s, feat, out, B, T, F, slice, *p, position_base,
                   (uint32_t)step, ex, plan_out);
    }
    KWS_LAUNCH_CHECK("feature_mask_kernel");
    return KWS_OK;
}

}  // extern "C"
