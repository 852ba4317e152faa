// csrc/kws_filter.h -- Butterworth filter augmentation of raw audio (the filtfilt of tools/audio_process/wav_filter.py of the reference,
// drawn per clip and per step on the device).  The bank layout and the chunk geometry shared by kws_filter.hip's kernel and host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kws.h"

namespace kws {
namespace flt {
// One wave per clip, lane = chunk: the padded clip (Lv + 2 padlen samples) is cut into 64 chunks of C = 2^m samples, m the smallest
// in [kMinLog, kMaxLog] that covers it.  The scan across lanes needs A^(C 2^j), j < 6, i.e. A^(2^e) for e <= kMaxLog + 5.
constexpr int kLanes = 64;
constexpr int kMinLog = 2;
constexpr int kMaxLog = 8;                     // C <= 256: 64 * 256 = 16384 >= KWS_FILTER_MAX_SAMPLES + 2 KWS_FILTER_MAX_PADLEN
constexpr int kPowers = kMaxLog + 6;           // A^(2^e), e = 0..13
constexpr int kMaxStates = 2 * KWS_FILTER_MAX_SECTIONS;
constexpr int kMat = kMaxStates * kMaxStates;  // doubles per stored power (row-major n x n, n = 2 n_sections, packed at the front)
constexpr int kCoef = 64;                      // doubles of coefficients per filter: (b0, b1, b2, -a1, -a2) per section, then zi[2 S]
constexpr int kStride = kCoef + kPowers * kMat;   // doubles per filter in the device table
static_assert(kLanes << kMaxLog >= KWS_FILTER_MAX_SAMPLES + 2 * KWS_FILTER_MAX_PADLEN, "chunks must cover the padded clip");
static_assert(2 * KWS_FILTER_MAX_PADLEN <= kLanes, "the two odd-extension edges live in one LDS float per lane");
}  // namespace flt
}  // namespace kws

struct kws_filter_bank {
    int K = 0;                     // filters
    int S = 0;                     // sections per filter (lower orders padded with identity sections)
    std::vector<int32_t> padlen;   // host copy
    int32_t *d_padlen = nullptr;   // [K]
    double *table = nullptr;       // [K][kStride]: coefficients, zi, then the powers of the state matrix (fp64)
};
