// csrc/kws_wave_stage.h -- what the raw-audio augmentation stages share (kws_speed.hip, kws_reverb.hip, kws_filter.hip, kws_augment.hip):
// a stage reads the B clips wav[index[b]] of valid_len samples, draws per clip at the clip's GLOBAL position in the batch, and writes
// float32 rows with zeros after the clip.  Device side: the sample conversion, the counter-based draws, the clip's source and the dry
// copy.  Host side: the argument checks the entry points have in common and the dispatch on the sample type.  A new stage starts here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "kws_common.h"

namespace kws {

// the featurizer's sample conversion (kws_featurize.hip: to_f32, data_utils.py:21)
__device__ __forceinline__ float aug_to_f32(float v) { return v; }
__device__ __forceinline__ float aug_to_f32(short v) { return (float)v * (1.0f / 32768.0f); }

// Counter-based draws (the mixing of dropout_keep, kws_device.h), keyed by (seed, step) and indexed by fields * position + field,
// position = the clip's GLOBAL position in the batch.  tests/aug_ref.py restates them in numpy.
__host__ __device__ inline uint32_t aug_hash(uint64_t seed, uint32_t step, uint32_t index)
{
    const uint32_t key_lo = (uint32_t)seed ^ (step * 0x27D4EB2Fu), key_hi = (uint32_t)(seed >> 32) + step;
    uint32_t h = index ^ key_lo;
    h += key_hi * 0x9E3779B9u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// uniform integer in [0, n)
__host__ __device__ inline uint32_t aug_uniform(uint32_t h, uint32_t n) { return (uint32_t)(((uint64_t)h * n) >> 32); }
// uniform float in [0, 1): the hash's upper 24 bits
__host__ __device__ inline float aug_unit(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }
// field 0 of clip b's draws
__device__ __forceinline__ uint32_t aug_pos(int64_t position_base, int b, int fields) { return (uint32_t)(position_base + b) * (uint32_t)fields; }
// with probability `rate` one of K (uniform), else -1: the fields f_apply and f_pick of the draws at pos
__device__ __forceinline__ int aug_pick(uint64_t seed, uint32_t step, uint32_t pos, int f_apply, int f_pick, float rate, int K)
{
    return aug_unit(aug_hash(seed, step, pos + f_apply)) < rate ? (int)aug_uniform(aug_hash(seed, step, pos + f_pick), (uint32_t)K) : -1;
}

// The source of clip b: its row of wav, its length clamped to [0, stride] (no valid_len: the whole row) and that length clipped to
// max_samples, which is the featurizer's clipping.  `len` is exact for stride <= INT_MAX (kws_speed_apply, its only reader, checks that).
struct ClipSrc {
    int row, len, clipped;
};
__device__ __forceinline__ ClipSrc clip_src(const int32_t *__restrict__ index, const int32_t *valid_len, int64_t stride, int max_samples, int b)
{
    ClipSrc c;
    c.row = index ? index[b] : b;
    int64_t l = valid_len ? (int64_t)valid_len[c.row] : stride;
    l = l < 0 ? 0 : l > stride ? stride : l;
    c.len = (int)l;
    c.clipped = l < max_samples ? (int)l : max_samples;
    return c;
}

// A clip the stage leaves as it is: the float32 conversion of its first lv samples, zeros up to out_stride.  Every thread of the block
// calls it; dst may be v itself (the filter in place), so neither is __restrict__.
template <int kThreads, typename WavT>
__device__ __forceinline__ void dry_copy(float *dst, const WavT *v, int lv, int64_t out_stride)
{
    const int tid = threadIdx.x;
    for (int t = tid; t < lv; t += kThreads) dst[t] = aug_to_f32(v[t]);
    for (int64_t t = (int64_t)lv + tid; t < out_stride; t += kThreads) dst[t] = 0.f;
}

// The argument checks of a stage's entry point that follow its null-pointer and own-parameter checks, in the order every stage has
// reported them.  max_cap: the stage's own limit on max_samples (INT_MAX: none); int_stride: the stage indexes a whole row with an int;
// out_stride: nullptr for a stage without `out`.
static inline int check_clip_batch(int max_samples, int max_cap, int B, int64_t stride, bool int_stride, const int32_t *valid_len,
                            int64_t position_base, const int64_t *out_stride, int wav_dtype)
{
    if (max_samples < 1) return fail(KWS_ERR_INVALID, "max_samples must be >= 1");
    if (max_samples > max_cap) return fail(KWS_ERR_UNSUPPORTED, "max_samples %d > %d", max_samples, max_cap);
    if (B < 0 || stride < 0 || position_base < 0) return fail(KWS_ERR_INVALID, "negative batch, stride or position_base");
    if (int_stride && stride > INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "stride %lld does not fit 31 bits", (long long)stride);
    if (!valid_len && stride < 1 && B > 0) return fail(KWS_ERR_INVALID, "stride must be >= 1 when valid_len is NULL");
    if (out_stride && *out_stride < max_samples) return fail(KWS_ERR_INVALID, "out_stride %lld < max_samples %d", (long long)*out_stride, max_samples);
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    return KWS_OK;
}

// f(WavT{}, "f32" / "i16" name) for the sample type of a checked wav_dtype: one launch site per kernel template
template <typename F>
inline int for_wav_type(int wav_dtype, const char *name_f32, const char *name_i16, F &&f)
{
    return wav_dtype == KWS_WAV_F32 ? f(float{}, name_f32) : f(short{}, name_i16);
}

}  // namespace kws
