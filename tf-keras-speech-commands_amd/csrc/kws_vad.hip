// csrc/kws_vad.hip -- voice-activity detection of whole recordings (include/kws.h: kws_vad_*; the `simple` detector of
// tools/audio_process/speech_duration_check.py:21-176 and the energy test of tools/audio_process/silent_check.py:14-24 of the reference).
//
// Two launches per call, no host synchronisation between them:
//
//   vad_ratio_kernel   grid (R, tiles), 256 threads.  A job is 64 consecutive HALF windows (H samples each) of one recording, which make
//                      63 windows (window w = halves w and w + 1; consecutive jobs share one half).  Wave v multiplies its 16 halves with
//                      the fixed (H x 112) cos/sin matrix of the band bins on v_mfma_f32_16x16x4_f32 (7 column tiles, 28 accumulator
//                      registers); the products P go to LDS, and X_k(w) = P_k(w) + (-1)^k P_k(w + 1) gives the band energy of a window
//                      from two LDS rows.  The total energy comes from Parseval, N sum x^2 - (sum x)^2 + (sum (-1)^n x_n)^2, with per-half
//                      sums that are exact 64-bit integers for int16 input (double for float32), so a DC offset cannot cancel in fp32.
//                      Every job also leaves the sum of squares of the samples it owns in a workspace slot: no atomics.
//   vad_smooth_kernel  grid R, 1024 threads.  A block walks its recording 1024 windows at a time: raw flags (ratio > threshold) with a
//                      halo in LDS, the majority of the 2 h + 1 flags around each window (ends replicated), begin / end events, and a
//                      block-level scan that numbers them, with the counts carried from chunk to chunk.  It also adds the recording's
//                      workspace slots in a fixed order for energy_per_second.
//   vad_gather_kernel  one block per clip: the cut, its padding and the 1/32768 scaling of the featurizer.
//
// A sample at or past lengths[r] is never used: every load is guarded by the recording's own length.
#include <climits>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "kws_common.h"
#include "kws_augment.h"
#include "kws_device.h"

struct kws_vad {
    int rate = 0, N = 0, H = 0, Kp = 0;      // window, hop (= half window), H rounded up to the K step of the product
    int bin_lo = 0, bin_hi = 0;              // band bins, inclusive
    int median = 0;                          // odd length of the smoothing median
    double threshold = 0.0;                  // a window is speech when band / full > threshold
    std::vector<float> mat;                  // [Kp][kCols]: column 2 i = cos, 2 i + 1 = sin of bin bin_lo + i; zero padding
    std::mutex mu;
    std::map<int, float *> dev;              // device id -> the matrix's copy there
};

namespace kws {
namespace vad {

constexpr int kThreads = 256, kTileH = 64, kTileW = kTileH - 1, kCols = 112, kColTiles = kCols / 16, kPStride = kCols + 1;
constexpr int kKStep = 16;                   // samples of one row a lane loads per step: 4 MFMAs of K = 4
constexpr int kSmoothThreads = 1024, kSmoothWaves = kSmoothThreads / 64, kMaxHalo = 127;

template <typename WavT> struct Sum;
template <> struct Sum<short> { typedef long long type; };
template <> struct Sum<float> { typedef double type; };

__device__ __forceinline__ long long raw_value(short v) { return (long long)v; }
__device__ __forceinline__ double raw_value(float v) { return (double)v; }
// the sums of int16 input are in units of 1 / 32768 (squares: 2^-30)
__device__ __forceinline__ double to_energy(long long v) { return (double)v * (1.0 / 1073741824.0); }
__device__ __forceinline__ double to_energy(double v) { return v; }

__host__ __device__ inline int window_count(int64_t L, int N, int H) { return L > N ? (int)((L - N + H - 1) / H) : 0; }
__host__ __device__ inline int tile_count(int n_windows) { return n_windows > kTileW ? (n_windows + kTileW - 1) / kTileW : 1; }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T *part, int tid, int waves)      // fixed order: butterfly in a wave, waves ascending
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    T total = part[0];
    for (int w = 1; w < waves; ++w) total += part[w];
    return total;
}

template <typename WavT>
__global__ __launch_bounds__(kThreads) void vad_ratio_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ lengths,
                                                             const float *__restrict__ mat, int N, int H, int Kp, int bin_lo,
                                                             int max_windows, int max_tiles, float *__restrict__ ratio,
                                                             typename Sum<WavT>::type *__restrict__ partial)
{
    typedef typename Sum<WavT>::type S;
    __shared__ float P[kTileH * kPStride];
    __shared__ S hs2[kTileH], hs1[kTileH], hsa[kTileH], part[kThreads / 64];
    const int r = blockIdx.x, job = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t L = lengths[r];
    L = L < 0 ? 0 : L > stride ? stride : L;
    const int n_win = window_count(L, N, H), n_tiles = tile_count(n_win), w0 = job * kTileW;
    float *rrow = ratio + (int64_t)r * max_windows;
    if (job >= n_tiles) {                                   // past the recording: zeros, nothing read
        if (tid < kTileW && w0 + tid < max_windows) rrow[w0 + tid] = 0.f;
        return;
    }
    const WavT *x = wav + (int64_t)r * stride;
    const int64_t s0 = (int64_t)w0 * H;                     // first sample of the job's first half

    // P = halves x matrix: lane l holds A[row l & 15][k = 4 (l >> 4) + j] for MFMA j of a step (the matrix rows are taken alike)
    {
        const int row = lane & 15, kg = lane >> 4;
        const int64_t rowbase = s0 + (int64_t)(16 * wave + row) * H;
        f32x4 acc[kColTiles];
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kp; k0 += kKStep) {
            const int kk = k0 + 4 * kg;
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t idx = rowbase + kk + j;
                a[j] = (kk + j < H && idx < L) ? aug_to_f32(x[idx]) : 0.f;
            }
            const float *b = mat + (int64_t)kk * kCols + row;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < kColTiles; ++t) acc[t] = mfma16(a[j], b[j * kCols + 16 * t], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < kColTiles; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) P[(16 * wave + 4 * kg + q) * kPStride + 16 * t + row] = acc[t][q];
    }
    // per-half sums for Parseval: four threads per half, samples k = part, part + 4, ...
    {
        const int half = tid >> 2, p4 = tid & 3;
        const int64_t base = s0 + (int64_t)half * H;
        S s2 = 0, s1 = 0, sa = 0;
        for (int k = p4; k < H; k += 4) {
            if (base + k < L) {
                const S v = raw_value(x[base + k]);
                s2 += v * v;
                s1 += v;
                sa += (k & 1) ? -v : v;
            }
        }
        s2 += __shfl_xor(s2, 1, 64); s1 += __shfl_xor(s1, 1, 64); sa += __shfl_xor(sa, 1, 64);
        s2 += __shfl_xor(s2, 2, 64); s1 += __shfl_xor(s1, 2, 64); sa += __shfl_xor(sa, 2, 64);
        if (p4 == 0) { hs2[half] = s2; hs1[half] = s1; hsa[half] = sa; }
    }
    __syncthreads();
    // windows: four threads per window, 28 columns each
    {
        const int w = tid >> 2, p4 = tid & 3, wc = w < kTileW ? w : kTileW - 1;
        const float *pa = P + wc * kPStride + p4 * (kCols / 4), *pb = pa + kPStride;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < kCols / 4; ++c) {
            const int bin = bin_lo + ((p4 * (kCols / 4) + c) >> 1);
            const float xk = (bin & 1) ? pa[c] - pb[c] : pa[c] + pb[c];
            s = __fmaf_rn(xk, xk, s);
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (p4 == 0 && w < kTileW && w0 + w < max_windows) {
            float out = 0.f;
            if (w0 + w < n_win) {
                const S S2 = hs2[w] + hs2[w + 1], S1 = hs1[w] + hs1[w + 1], SA = hsa[w] + ((H & 1) ? -hsa[w + 1] : hsa[w + 1]);
                const double full = to_energy((S)N * S2 - S1 * S1 + SA * SA);
                if (full > 0.0) out = (float)(2.0 * (double)s / full);
            }
            rrow[w0 + w] = out;
        }
    }
    // the job's own samples: halves 0 .. 62, and for the recording's last job everything after them
    {
        S q = tid < kTileW ? hs2[tid] : (S)0;
        if (job == n_tiles - 1)
            for (int64_t i = s0 + (int64_t)kTileW * H + tid; i < L; i += kThreads) {
                const S v = raw_value(x[i]);
                q += v * v;
            }
        const S total = block_sum(q, part, tid, kThreads / 64);
        if (tid == 0) partial[(int64_t)r * max_tiles + job] = total;
    }
}

template <typename S>
__global__ __launch_bounds__(kSmoothThreads) void vad_smooth_kernel(const float *__restrict__ ratio, const int32_t *__restrict__ lengths,
                                                                    int64_t stride, int N, int H, int halo, double threshold, int rate,
                                                                    int max_windows, int max_tiles, int max_segments,
                                                                    const S *__restrict__ partial, uint8_t *__restrict__ smoothed,
                                                                    int32_t *__restrict__ segments, int32_t *__restrict__ n_segments,
                                                                    int32_t *__restrict__ span, double *__restrict__ energy_per_second)
{
    constexpr int T = kSmoothThreads;
    __shared__ uint8_t raw[T + 2 * kMaxHalo], sm[T + 1];
    __shared__ uint32_t wave_tot[kSmoothWaves];
    __shared__ int32_t first_begin, last_end, base_b, base_e;
    __shared__ S part[kSmoothWaves];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t L = lengths[r];
    L = L < 0 ? 0 : L > stride ? stride : L;
    const int n_win = window_count(L, N, H), n_tiles = tile_count(n_win);
    const float *rrow = ratio + (int64_t)r * max_windows;
    uint8_t *srow = smoothed + (int64_t)r * max_windows;
    int32_t *seg = segments + (int64_t)r * max_segments * 2;
    if (tid == 0) { first_begin = 0; last_end = 0; base_b = 0; base_e = 0; sm[0] = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < n_win; c0 += T) {
        for (int i = tid; i < T + 2 * halo; i += T) {                      // raw flags of [c0 - halo, c0 + T + halo), ends replicated
            int w = c0 - halo + i;
            w = w < 0 ? 0 : w >= n_win ? n_win - 1 : w;
            raw[i] = (double)rrow[w] > threshold ? 1 : 0;
        }
        __syncthreads();
        const int w = c0 + tid;
        const bool live = w < n_win;
        int s = 0;
        if (live) {
            int cnt = 0;
            for (int d = 0; d <= 2 * halo; ++d) cnt += raw[tid + d];
            s = cnt > halo ? 1 : 0;
            srow[w] = (uint8_t)s;
        }
        sm[tid + 1] = (uint8_t)s;
        __syncthreads();
        const int prev = sm[tid];
        const uint32_t b = live && s && !prev, e = live && !s && prev;
        uint32_t v = b | (e << 16), inc = v;                               // begins in the low half, ends in the high half
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int q = 0; q < kSmoothWaves; ++q) {
            if (q < wave) before += wave_tot[q];
            total += wave_tot[q];
        }
        const uint32_t excl = before + inc - v;
        const int bi = base_b + (int)(excl & 0xffffu), ei = base_e + (int)(excl >> 16);
        const int32_t at = (int32_t)((int64_t)w * H);
        if (b) {
            if (bi < max_segments) seg[2 * bi] = at;
            if (bi == 0) first_begin = at;
        }
        if (e) {
            if (ei < max_segments) seg[2 * ei + 1] = at;
            atomicMax(&last_end, at);
        }
        const int last = sm[T];
        __syncthreads();
        if (tid == 0) { base_b += (int)(total & 0xffffu); base_e += (int)(total >> 16); sm[0] = (uint8_t)last; }
        __syncthreads();
    }
    for (int w = n_win + tid; w < max_windows; w += T) srow[w] = 0;
    const int n_seg = base_e;                                              // an interval still open at the last window is dropped
    for (int i = (n_seg < max_segments ? n_seg : max_segments) * 2 + tid; i < 2 * max_segments; i += T) seg[i] = 0;
    S q = 0;
    for (int j = tid; j < n_tiles; j += T) q += partial[(int64_t)r * max_tiles + j];
    const S total = block_sum(q, part, tid, kSmoothWaves);
    if (tid == 0) {
        n_segments[r] = n_seg;
        span[2 * r] = n_seg > 0 ? first_begin : 0;
        span[2 * r + 1] = n_seg > 0 ? last_end : 0;
        energy_per_second[r] = L > 0 ? to_energy(total) / ((double)L / (double)rate) : 0.0;
    }
}

template <typename WavT>
__global__ __launch_bounds__(kThreads) void vad_gather_kernel(const WavT *__restrict__ wav, int R, int64_t stride,
                                                              const int32_t *__restrict__ lengths, const int32_t *__restrict__ triples,
                                                              int clip_samples, int pad_before, int pad_after, int align,
                                                              float *__restrict__ clips)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int rec = triples[3 * b];
    float *dst = clips + (int64_t)b * clip_samples;
    int64_t lo = 0, keep = 0;
    if (rec >= 0 && rec < R) {
        int64_t L = lengths[rec];
        L = L < 0 ? 0 : L > stride ? stride : L;
        lo = (int64_t)triples[3 * b + 1] - pad_before;
        int64_t hi = (int64_t)triples[3 * b + 2] + pad_after;
        lo = lo < 0 ? 0 : lo;
        hi = hi > L ? L : hi;
        keep = hi > lo ? hi - lo : 0;
        keep = keep > clip_samples ? clip_samples : keep;                  // a longer cut keeps its head
    }
    const int64_t off = align == 0 ? clip_samples - keep : (clip_samples - keep) / 2;
    const WavT *x = wav + (int64_t)(rec >= 0 && rec < R ? rec : 0) * stride + lo - off;
    for (int i = tid; i < clip_samples; i += kThreads) dst[i] = (i >= off && i < off + keep) ? aug_to_f32(x[i]) : 0.f;
}

// the matrix's copy on the current device
int device_matrix(const kws_vad *vd, const float **out)
{
    kws_vad *m = const_cast<kws_vad *>(vd);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KWS_ERR_HIP, "voice-activity detection needs a HIP device; there is no CPU fallback");
    }
    std::lock_guard<std::mutex> lk(m->mu);
    float *&d = m->dev[dev];
    if (!d) {
        const size_t bytes = sizeof(float) * m->mat.size();
        if (hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
            return fail(KWS_ERR_HIP, "vad: device allocation of %zu bytes failed (no HIP device? there is no CPU fallback)", bytes);
        }
        if (hipMemcpy(d, m->mat.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d);
            d = nullptr;
            return fail(KWS_ERR_HIP, "vad: upload of the cos/sin matrix failed");
        }
    }
    *out = d;
    return KWS_OK;
}

inline int max_tiles_of(int max_windows) { return tile_count(max_windows); }

}  // namespace vad
}  // namespace kws

using namespace kws;
using namespace kws::vad;

extern "C" {

int kws_vad_create(int sample_rate, double window_t, double hop_t, double band_lo, double band_hi, double energy_threshold,
                   double smooth_t, kws_vad **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (sample_rate < 1 || !(window_t > 0.0) || !(hop_t > 0.0) || !(smooth_t > 0.0))
        return fail(KWS_ERR_INVALID, "sample_rate, window_t, hop_t and smooth_t must be positive");
    if (!(band_lo >= 0.0 && band_hi > band_lo)) return fail(KWS_ERR_INVALID, "the band [%g, %g] Hz is empty", band_lo, band_hi);
    if (!(energy_threshold >= 0.0 && energy_threshold < 1.0))
        return fail(KWS_ERR_INVALID, "energy_threshold %g is outside [0, 1)", energy_threshold);
    const double dn = (double)sample_rate * window_t, dh = (double)sample_rate * hop_t;
    if (dn > 1e6 || dh > 1e6) return fail(KWS_ERR_UNSUPPORTED, "a window of %g samples is not supported", dn);
    const int N = (int)dn, H = (int)dh;                       // int(rate * t), speech_duration_check.py:156-157
    if (H < 1 || N != 2 * H || N > 1024)
        return fail(KWS_ERR_UNSUPPORTED,
                    "sample rate %d gives a window of %d and a hop of %d samples: only window == 2 * hop with window <= 1024 is supported",
                    sample_rate, N, H);
    int median = (int)(smooth_t / window_t);                  // speech_duration_check.py:103-104
    if (median % 2 == 0) median -= 1;
    if (median < 1 || (median - 1) / 2 > kMaxHalo)
        return fail(KWS_ERR_UNSUPPORTED, "a median of %d windows is outside [1, %d]", median, 2 * kMaxHalo + 1);
    // np.fft.fftfreq(N, 1 / rate)[k] = k * (1 / (N * (1 / rate))); the band keeps lo < f < hi among k = 1 .. N / 2
    const double val = 1.0 / ((double)N * (1.0 / (double)sample_rate));
    int lo = 0, hi = -1;
    for (int k = 1; k <= N / 2; ++k) {
        const double f = (double)k * val;
        if (band_lo < f && f < band_hi) {
            if (hi < 0) lo = k;
            hi = k;
        }
    }
    if (hi < 0) return fail(KWS_ERR_UNSUPPORTED, "no frequency bin of the %d-point window lies inside (%g, %g) Hz", N, band_lo, band_hi);
    if (2 * (hi - lo + 1) > kCols)
        return fail(KWS_ERR_UNSUPPORTED, "the band holds %d bins, more than the %d the kernel's matrix has room for", hi - lo + 1, kCols / 2);
    auto *vd = new kws_vad();
    vd->rate = sample_rate;
    vd->N = N;
    vd->H = H;
    vd->Kp = (H + kKStep - 1) / kKStep * kKStep;
    vd->bin_lo = lo;
    vd->bin_hi = hi;
    vd->median = median;
    vd->threshold = energy_threshold;
    vd->mat.assign((size_t)vd->Kp * kCols, 0.f);
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < H; ++n)
        for (int k = lo; k <= hi; ++k) {
            const int m = (int)(((int64_t)k * n) % N);        // exact phase reduction
            const double ang = 2.0 * pi * (double)m / (double)N;
            vd->mat[(size_t)n * kCols + 2 * (k - lo)] = (float)std::cos(ang);
            vd->mat[(size_t)n * kCols + 2 * (k - lo) + 1] = (float)std::sin(ang);
        }
    *out = vd;
    return KWS_OK;
}

void kws_vad_destroy(kws_vad *vd)
{
    if (!vd) return;
    for (auto &kv : vd->dev)
        if (kv.second) (void)hipFree(kv.second);
    delete vd;
}

int kws_vad_info(const kws_vad *vd, int32_t *window_samples, int32_t *hop_samples, int32_t *bin_lo, int32_t *bin_hi, int32_t *median)
{
    if (!vd) return fail(KWS_ERR_INVALID, "null argument");
    if (window_samples) *window_samples = vd->N;
    if (hop_samples) *hop_samples = vd->H;
    if (bin_lo) *bin_lo = vd->bin_lo;
    if (bin_hi) *bin_hi = vd->bin_hi;
    if (median) *median = vd->median;
    return KWS_OK;
}

int64_t kws_vad_windows(const kws_vad *vd, int64_t n_samples)
{
    if (!vd) return fail(KWS_ERR_INVALID, "null argument");
    if (n_samples < 0 || n_samples > INT_MAX) return fail(KWS_ERR_INVALID, "n_samples %lld is outside an int32 sample count", (long long)n_samples);
    return window_count(n_samples, vd->N, vd->H);
}

int64_t kws_vad_workspace_bytes(const kws_vad *vd, int R, int max_windows)
{
    if (!vd) return fail(KWS_ERR_INVALID, "null argument");
    if (R < 0 || max_windows < 0) return fail(KWS_ERR_INVALID, "negative R / max_windows");
    return (int64_t)sizeof(double) * (int64_t)(R > 0 ? R : 1) * max_tiles_of(max_windows);
}

int kws_vad_detect(const kws_vad *vd, const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths, int max_windows,
                   int max_segments, void *workspace, int64_t workspace_bytes, float *ratio, uint8_t *smoothed, int32_t *segments,
                   int32_t *n_segments, int32_t *span, double *energy_per_second, void *stream)
{
    if (!vd) return fail(KWS_ERR_INVALID, "null argument");
    if (R < 0 || max_windows < 0 || max_segments < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative R / max_windows / max_segments / stride");
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    if (stride > INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "stride %lld does not fit 31 bits", (long long)stride);
    if (R == 0) return KWS_OK;
    if (!lengths || !n_segments || !span || !energy_per_second || !workspace || (stride > 0 && !wav)) return fail(KWS_ERR_INVALID, "null argument");
    if (max_windows > 0 && (!ratio || !smoothed)) return fail(KWS_ERR_INVALID, "null argument");
    if (max_segments > 0 && !segments) return fail(KWS_ERR_INVALID, "null argument");
    if (max_windows < window_count(stride, vd->N, vd->H))
        return fail(KWS_ERR_INVALID, "max_windows=%d is fewer than the %d windows a recording of stride %lld samples can have", max_windows,
                    window_count(stride, vd->N, vd->H), (long long)stride);
    const int max_tiles = max_tiles_of(max_windows);
    if (max_tiles > 65535) return fail(KWS_ERR_UNSUPPORTED, "max_windows=%d needs more than 65535 tiles of %d windows", max_windows, kTileW);
    if (max_segments > (INT_MAX - 1) / 2) return fail(KWS_ERR_INVALID, "max_segments=%d is too large", max_segments);
    const int64_t need = kws_vad_workspace_bytes(vd, R, max_windows);
    if (workspace_bytes < need) return fail(KWS_ERR_WORKSPACE, "workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return fail(KWS_ERR_INVALID, "the workspace must be 8-byte aligned");
    const float *mat = nullptr;
    if (int rc = device_matrix(vd, &mat)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)R, (unsigned)max_tiles);
    const int halo = (vd->median - 1) / 2;
    if (wav_dtype == KWS_WAV_I16) {
        KWS_LAUNCH("vad_ratio_i16", (vad_ratio_kernel<short>), grid, dim3(kThreads), 0, s, static_cast<const short *>(wav), stride, lengths, mat,
                   vd->N, vd->H, vd->Kp, vd->bin_lo, max_windows, max_tiles, ratio, static_cast<long long *>(workspace));
        KWS_LAUNCH_CHECK("vad_ratio_kernel");
        KWS_LAUNCH("vad_smooth", (vad_smooth_kernel<long long>), dim3((unsigned)R), dim3(kSmoothThreads), 0, s, ratio, lengths, stride, vd->N,
                   vd->H, halo, vd->threshold, vd->rate, max_windows, max_tiles, max_segments, static_cast<const long long *>(workspace),
                   smoothed, segments, n_segments, span, energy_per_second);
    } else {
        KWS_LAUNCH("vad_ratio_f32", (vad_ratio_kernel<float>), grid, dim3(kThreads), 0, s, static_cast<const float *>(wav), stride, lengths, mat,
                   vd->N, vd->H, vd->Kp, vd->bin_lo, max_windows, max_tiles, ratio, static_cast<double *>(workspace));
        KWS_LAUNCH_CHECK("vad_ratio_kernel");
        KWS_LAUNCH("vad_smooth", (vad_smooth_kernel<double>), dim3((unsigned)R), dim3(kSmoothThreads), 0, s, ratio, lengths, stride, vd->N,
                   vd->H, halo, vd->threshold, vd->rate, max_windows, max_tiles, max_segments, static_cast<const double *>(workspace),
                   smoothed, segments, n_segments, span, energy_per_second);
    }
    KWS_LAUNCH_CHECK("vad_smooth_kernel");
    return KWS_OK;
}

int kws_vad_gather_clips(const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths, const int32_t *triples, int n,
                         int clip_samples, int pad_before, int pad_after, int align, float *clips, void *stream)
{
    if (R < 0 || n < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative R / n / stride");
    if (clip_samples < 1) return fail(KWS_ERR_INVALID, "clip_samples must be >= 1");
    if (pad_before < 0 || pad_after < 0) return fail(KWS_ERR_INVALID, "pad_before and pad_after must be >= 0");
    if (align != KWS_VAD_ALIGN_LEFT_PAD && align != KWS_VAD_ALIGN_CENTER) return fail(KWS_ERR_INVALID, "unknown clip alignment %d", align);
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    if (stride > INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "stride %lld does not fit 31 bits", (long long)stride);
    if (n == 0) return KWS_OK;
    if (!lengths || !triples || !clips || (stride > 0 && !wav)) return fail(KWS_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (wav_dtype == KWS_WAV_I16)
        KWS_LAUNCH("vad_gather_i16", (vad_gather_kernel<short>), dim3((unsigned)n), dim3(kThreads), 0, s, static_cast<const short *>(wav), R,
                   stride, lengths, triples, clip_samples, pad_before, pad_after, align, clips);
    else
        KWS_LAUNCH("vad_gather_f32", (vad_gather_kernel<float>), dim3((unsigned)n), dim3(kThreads), 0, s, static_cast<const float *>(wav), R,
                   stride, lengths, triples, clip_samples, pad_before, pad_after, align, clips);
    KWS_LAUNCH_CHECK("vad_gather_kernel");
    return KWS_OK;
}

}  // extern "C"
