// csrc/kws_reverb.h -- room-reverberation augmentation of raw audio (the convolution of tools/audio_process/audio_reverberation.py and
// gpuRIR_reverberation.py of the reference with a room impulse response, drawn per clip and per step on the device).  The bank and the
// transform geometry shared by kws_reverb.hip and its host-side spectrum code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kws.h"

namespace kws {
namespace rv {
// One transform size for every bank: a real FFT of N = 32768 points, done as a complex FFT of M = N / 2 points.  A clip and a clipped
// RIR are both at most 16384 samples, so their linear convolution (<= 32767 samples) never wraps.
constexpr int kMaxSamples = 16384;
constexpr int N = 32768;
constexpr int M = N / 2;
constexpr int kSpecStride = M + 16;   // float2 per bank spectrum: H[0..M] and padding (keeps rows 128-byte aligned)
}  // namespace rv
}  // namespace kws

struct kws_rir_bank {
    int K = 0;                 // RIRs
    int max_samples = 0;       // taps at index >= max_samples are clipped away
    std::vector<int32_t> len;  // clipped lengths Lh (host)
    int32_t *d_len = nullptr;  // [K] device copy
    float2 *spec = nullptr;    // [K][kSpecStride]: H_k[0..M] / (4 M), fp64-computed, rounded to fp32 (the 1 / (4 M) folds every
                               // normalisation of the real-FFT packing and the inverse transform into the spectrum; a power of two)
    float *taps = nullptr;     // [K][max_samples]: the clipped taps, zeros after Lh (clips of a few samples are convolved directly)
    float2 *tw = nullptr;      // [N] exp(-2 pi i n / N), fp64-computed, rounded to fp32
};
