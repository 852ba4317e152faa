// csrc/kws_resample.h -- the band-limited interpolation of include/kws.h's speed section, shared by the two stages that resample
// (kws_speed.hip: the speed change; kws_pitch.hip: the pitch shift behind the phase vocoder): the table's owner and one output sample.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "kws_common.h"
#include "kws_wave_stage.h"

struct kws_resampler {
    int Z = 0, P = 0;
    double beta = 0.0, rolloff = 0.0;
    std::vector<float> table;            // h[0 .. Z P]
    std::mutex mu;
    std::map<int, float *> dev;          // device id -> the table's copy there (made by the first kws_speed_apply on that device)
};

namespace kws {
namespace spd {

constexpr size_t kMaxTableBytes = 64 * 1024;

// the table's copy on the current device (kws_speed.hip)
int device_table(const kws_resampler *rs, const float **out);

// one wing of output n: taps at v[j], j = j0, j0 + dj, ... while 0 <= j < Ls and pos = ((x0 + k) s) P < Z P
template <typename WavT>
__device__ __forceinline__ float wing(const WavT *__restrict__ v, const float *h, int j0, int dj, int Ls, double x0, double s, double dP,
                                      double lim, float acc)
{
#pragma clang fp contract(off)
    double k = 0.0;
    for (int j = j0; j >= 0 && j < Ls; j += dj, k += 1.0) {
        const double pos = ((x0 + k) * s) * dP;
        if (!(pos < lim)) break;
        const int i = (int)pos;
        const float eta = (float)(pos - (double)i);
        const float h0 = h[i], h1 = h[i + 1];
        acc = __fmaf_rn(__fmaf_rn(eta, h1 - h0, h0), aug_to_f32(v[j]), acc);
    }
    return acc;
}

// output n of the clip v[0 .. Ls) played rd times faster: s = min(1, 1 / rd), sf = (float)s, dP = P, lim = Z P, h the table (in LDS)
template <typename WavT>
__device__ __forceinline__ float resample_at(const WavT *__restrict__ v, const float *h, int n, int Ls, double rd, double s, float sf,
                                             double dP, double lim)
{
    const double t = (double)n * rd, f0 = floor(t), phi = t - f0;   // n r is exact: 15 x 24 bits
    const int n0 = (int)f0;
    float acc = wing(v, h, n0, -1, Ls, phi, s, dP, lim, 0.f);
    acc = wing(v, h, n0 + 1, 1, Ls, 1.0 - phi, s, dP, lim, acc);
    return sf * acc;
}

}  // namespace spd
}  // namespace kws
