// csrc/kws_augment.h -- background-noise augmentation of raw audio (the mix of tools/audio_process/add_noise.py:19-35 of the reference,
// redrawn per clip and per step on the device).  Shared by kws_augment.hip (noise bank, plan and apply kernels) and kws_featurize.hip
// (the fused instantiation of the tuned featurizer): both build a sample of the mixed clip with aug_sample() below, so the fused
// featurizer and featurize(apply(...)) see the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kws.h"
#include "kws_wave_stage.h"

struct kws_noise_bank {
    int K = 0;                 // segments (recordings)
    int64_t total = 0;         // samples over all segments
    std::vector<int64_t> start;   // host copies of the tables
    std::vector<int32_t> len;
    float *samples = nullptr;  // [total] float32 (int16 banks are scaled by 1/32768 on upload, as the featurizer's to_f32)
    int64_t *d_start = nullptr;   // [K]
    int32_t *d_len = nullptr;     // [K]
    double *prefix = nullptr;     // [total + 1] prefix sums of squares: the power of any window in O(1)
};

namespace kws {

// what the fused featurizer needs per clip: the plan records and the bank
struct AugDev {
    const kws_aug_clip *plan;
    const float *bank;
    const int64_t *seg_start;
};

// Sample t of the clip the featurizer sees: m'[t] = m[t - d] for 0 <= t - d < L (0 elsewhere and for t outside [0, L)), with
// m[u] = v[u] + g * n[u] when the clip is noised (n = the noise window, already offset), else v[u].  One explicit fused multiply-add, so
// no surrounding code can contract it differently.
template <typename WavT>
__device__ __forceinline__ float aug_sample(const WavT *__restrict__ v, const float *__restrict__ n, int L, int d, float g, bool noised, int t)
{
    const int u = t - d;
    float x = 0.f;
    if (t >= 0 && t < L && u >= 0 && u < L) {
        x = aug_to_f32(v[u]);
        if (noised) x = __fmaf_rn(g, n[u], x);
    }
    return x;
}

// the draw fields of a clip: aug_hash(seed, step, 5 * position + field) (kws_wave_stage.h)
enum { kAugApply = 0, kAugSegment = 1, kAugSnr = 2, kAugOffset = 3, kAugShift = 4, kAugFields = 5 };

// featurize(apply(...)) for the featurizer configurations without a fused path (kws_augment.hip)
int augment_apply_launch(const kws_noise_bank *bank, const kws_aug_clip *plan, const void *wav, int wav_dtype, const int32_t *index, int B,
                         int64_t stride, int max_samples, float *out, int64_t out_stride, int32_t *lengths, hipStream_t s);

}  // namespace kws
