// csrc/kws_rate.hip -- sample-rate conversion in front of the detector (include/kws.h: kws_rate_*): the polyphase bank, a host object,
// and the one kernel that serves both the streaming form (per-stream history rows) and the one-shot form (whole recordings as rows).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "kws_common.h"

struct kws_rate_bank {
    int f_in = 0, f_out = 0, p = 0, q = 0, K = 0, Z = 0;
    double beta = 0.0, rolloff = 0.0;
    std::vector<float> w;                // (q, 2K) row-major
    std::mutex mu;
    std::map<int, float *> dev;          // device id -> the bank's tap-major copy there, (2K, q)
};

namespace kws {
namespace spd {
double bessel_i0(double x);              // kws_speed.hip
}
namespace rate {

constexpr int kThreads = 256;
constexpr int kTile = 512;               // outputs of one block: two per lane
constexpr int kLdsPhases = 4;            // banks of at most this many phases are staged in LDS (8 / 32 / 48 / 64 kHz <-> 16 kHz)
constexpr int kLdsBankFloats = 2 * 128 * kLdsPhases;      // K <= ceil(32 * 4) = 128
constexpr int kMaxTilesY = 65535;
constexpr int64_t kMaxN = (int64_t)1 << 44;

struct BankDev {
    const float *w;                      // (2K, q)
    int p, q, K, pad;
};
struct Banks {
    BankDev b[KWS_RATE_MAX_BANKS];
};

// samples a tile stages: the taps of its first output's left wing through its last output's right wing
inline int tile_span(int p, int q, int K) { return (int)(((int64_t)(q - 1) + (int64_t)(kTile - 1) * p) / q) + 2 * K; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One output: the left wing from s[0] down, the right wing from s[1] up, in the order of include/kws.h.  w points at phase m of tap 0,
// taps lie q apart.
__device__ __forceinline__ float one_output(const float *w, const float *s, int q, int K)
{
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = __fmaf_rn(w[(size_t)k * q], s[-k], acc);
    w += (size_t)K * q;
    for (int k = 0; k < K; ++k) acc = __fmaf_rn(w[(size_t)k * q], s[1 + k], acc);
    return acc;
}

__device__ __forceinline__ void store_output(short *o16, float *o32, long at, float y)
{
    if (o32) o32[at] = y;
    if (o16) {
        const float r = rintf(y * 32768.f);
        o16[at] = (short)(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
    }
}

// grid (A, tiles): block (a, t) writes columns [t kTile, (t + 1) kTile) of entry a's output row, its outputs first, zeros to out_width
__global__ __launch_bounds__(kThreads) void rate_convert_kernel(Banks banks, int n_banks, const short *__restrict__ in, long in_stride,
                                                                int in_rows, const int *__restrict__ table, short *hist, long hist_stride,
                                                                int hist_rows, short *__restrict__ out_i16, float *__restrict__ out_f32,
                                                                long out_stride, int out_rows, int out_width, int span_cap)
{
    extern __shared__ float lds[];       // span_cap samples, then kLdsBankFloats weights
    const int tid = threadIdx.x;
    const int *e = table + (size_t)blockIdx.x * KWS_RATE_FIELDS;
    const int bi = e[KWS_RATE_BANK], out_row = e[KWS_RATE_OUT_ROW];
    if (bi < 0 || bi >= n_banks) return;                                                 // uniform over the block
    const bool has_out = out_row >= 0 && out_row < out_rows;                             // an entry may only feed its history
    const BankDev bk = banks.b[bi];
    const int p = bk.p, q = bk.q, K = bk.K, Hn = K > 0 ? 2 * K - 1 : 0;
    const int in_row = e[KWS_RATE_IN_ROW], flags = e[KWS_RATE_FLAGS];
    const int len = (in_row < 0 || in_row >= in_rows) ? 0 : clampi(e[KWS_RATE_IN_LEN], 0, (int)(in_stride > 0x7fffffffL ? 0x7fffffffL : in_stride));
    int64_t N = (int64_t)(uint32_t)e[KWS_RATE_N_LO] | ((int64_t)e[KWS_RATE_N_HI] << 32);
    int64_t first = (int64_t)(uint32_t)e[KWS_RATE_FIRST_LO] | ((int64_t)e[KWS_RATE_FIRST_HI] << 32);
    N = N < 0 ? 0 : (N > kMaxN ? kMaxN : N);
    first = first < 0 ? 0 : (first > kMaxN ? kMaxN : first);
    const int count = has_out ? clampi(e[KWS_RATE_COUNT], 0, out_width) : 0;
    const bool restart = (flags & KWS_RATE_RESTART) != 0;
    int hist_in = e[KWS_RATE_HIST_IN], hist_out = e[KWS_RATE_HIST_OUT];
    if (restart || hist_in < 0 || hist_in >= hist_rows || !hist) hist_in = -1;
    if ((flags & KWS_RATE_FINAL) || hist_out < 0 || hist_out >= hist_rows || !hist || hist_out == hist_in) hist_out = -1;
    const short *src = in + (size_t)(len > 0 ? in_row : 0) * in_stride;
    const short *hin = hist_in >= 0 ? hist + (size_t)hist_in * hist_stride : nullptr;

    // the stream's last 2K - 1 samples after this chunk: old history shifted by len, then the chunk (the entry's first block writes them)
    if (blockIdx.y == 0 && hist_out >= 0) {
        short *hout = hist + (size_t)hist_out * hist_stride;
        for (int i = tid; i < Hn; i += kThreads) {
            const int64_t c = (int64_t)i + len - Hn;                                     // position in the chunk, negative: in the history
            short v = 0;
            if (c >= 0) v = src[c];
            else if (hin) v = hin[i + len];
            hout[i] = v;
        }
    }

    if (!has_out) return;
    const int c0 = blockIdx.y * kTile;
    const int c1 = min(c0 + kTile, out_width);
    const int cn = min(c1, count) - c0;                                                  // outputs of this tile, <= 0: zeros only
    short *o16 = out_i16 ? out_i16 + (size_t)out_row * out_stride : nullptr;
    float *o32 = out_f32 ? out_f32 + (size_t)out_row * out_stride : nullptr;
    for (int c = max(c0, count) + tid; c < c1; c += kThreads) {
        if (o32) o32[c] = 0.f;
        if (o16) o16[c] = 0;
    }
    if (cn <= 0) return;

    if (K == 0) {                                                                        // p == q: the samples pass through
        for (int c = c0 + tid; c < c0 + cn; c += kThreads) {
            const int64_t j = first + c - N;
            const short v = (j >= 0 && j < len) ? src[j] : (short)0;
            if (o32) o32[c] = (float)v * (1.f / 32768.f);
            if (o16) o16[c] = v;
        }
        return;
    }

    // the tile's first output n = first + c0 sits at n0b, phase mb; output c0 + i at n0b + (mb + i p) / q, phase (mb + i p) mod q
    const int64_t t0 = (first + c0) * (int64_t)p;
    const int64_t n0b = t0 / q;
    const unsigned mb = (unsigned)(t0 - n0b * q);
    const int span = min(2 * K + (int)((mb + (unsigned)(cn - 1) * (unsigned)p) / (unsigned)q), span_cap);
    const int64_t jlo = n0b - (K - 1);                                                   // stream index of lds[0]
    for (int i = tid; i < span; i += kThreads) {
        const int64_t c = jlo + i - N;                                                   // position in the chunk
        short v = 0;
        if (c >= 0) { if (c < len) v = src[c]; }
        else if (hin && c + Hn >= 0) v = hin[c + Hn];
        lds[i] = (float)v * (1.f / 32768.f);
    }
    const bool staged = q <= kLdsPhases && 2 * K * q <= kLdsBankFloats;
    float *wl = lds + span_cap;
    if (staged)
        for (int i = tid; i < 2 * K * q; i += kThreads) wl[i] = bk.w[i];
    __syncthreads();

    for (int i = tid; i < cn; i += kThreads) {
        const unsigned u = mb + (unsigned)i * (unsigned)p;
        const unsigned dn = u / (unsigned)q, m = u - dn * (unsigned)q;
        const int at = K - 1 + (int)dn;                                                  // lds index of v[n0]
        float y = 0.f;
        if (at + K < span)                                                               // always, unless span_cap cut the span
            y = staged ? one_output(wl + m, lds + at, q, K) : one_output(bk.w + m, lds + at, q, K);
        store_output(o16, o32, (long)c0 + i, y);
    }
}

// the bank's tap-major copy on the current device
int device_bank(const kws_rate_bank *bank, const float **out)
{
    kws_rate_bank *m = const_cast<kws_rate_bank *>(bank);
    *out = nullptr;
    if (m->K == 0) return KWS_OK;
    int dev = 0;
    KWS_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(m->mu);
    float *&d = m->dev[dev];
    if (!d) {
        const int q = m->q, T = 2 * m->K;
        std::vector<float> t((size_t)q * T);
        for (int r = 0; r < q; ++r)
            for (int k = 0; k < T; ++k) t[(size_t)k * q + r] = m->w[(size_t)r * T + k];
        const size_t bytes = sizeof(float) * t.size();
        if (hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
            return fail(KWS_ERR_HIP, "rate bank: device allocation of %zu bytes failed", bytes);
        }
        if (hipMemcpy(d, t.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d);
            d = nullptr;
            return fail(KWS_ERR_HIP, "rate bank: upload failed");
        }
    }
    *out = d;
    return KWS_OK;
}

int64_t gcd64(int64_t a, int64_t b)
{
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

}  // namespace rate
}  // namespace kws

using namespace kws;
using namespace kws::rate;

extern "C" {

int kws_rate_bank_create(int f_in, int f_out, int zero_crossings, double beta, double rolloff, kws_rate_bank **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (f_in < 1 || f_out < 1) return fail(KWS_ERR_INVALID, "sample rates must be positive, got %d -> %d", f_in, f_out);
    if (zero_crossings < 4 || zero_crossings > 32) return fail(KWS_ERR_INVALID, "zero_crossings %d is outside [4, 32]", zero_crossings);
    if (!(beta >= 0.0 && beta <= 20.0)) return fail(KWS_ERR_INVALID, "beta %g is outside [0, 20]", beta);
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(KWS_ERR_INVALID, "rolloff %g is outside (0, 1]", rolloff);
    const int64_t g = gcd64(f_in, f_out), p = f_in / g, q = f_out / g, Z = zero_crossings;
    if (p > 4 * q || q > 4 * p)
        return fail(KWS_ERR_UNSUPPORTED, "%d Hz -> %d Hz: the ratio %lld / %lld is outside [1/4, 4]", f_in, f_out, (long long)p, (long long)q);
    const int64_t K = p == q ? 0 : (p < q ? Z : (Z * p + q - 1) / q);
    const int64_t bytes = q * 2 * K * (int64_t)sizeof(float);
    if (bytes > KWS_RATE_MAX_BANK_BYTES)
        return fail(KWS_ERR_UNSUPPORTED, "%d Hz -> %d Hz: a bank of %lld phases x %lld taps (%lld bytes) exceeds %d bytes", f_in, f_out,
                    (long long)q, (long long)(2 * K), (long long)bytes, (int)KWS_RATE_MAX_BANK_BYTES);
    auto *b = new kws_rate_bank();
    b->f_in = f_in; b->f_out = f_out; b->p = (int)p; b->q = (int)q; b->K = (int)K; b->Z = zero_crossings;
    b->beta = beta; b->rolloff = rolloff;
    b->w.assign((size_t)(q * 2 * K), 0.f);
    const double pi = 3.14159265358979323846, i0b = spd::bessel_i0(beta);
    const int64_t den = p > q ? p : q;                        // s d / q = d / max(p, q) for the integer distance d (in units of 1 / q)
    const double s = p > q ? (double)q / (double)p : 1.0;
    auto weight = [&](int64_t d) -> float {
        if (d >= Z * den) return 0.f;                         // h is 0 from Z on
        const double x = (double)d / (double)den, xr = rolloff * x, u = x / (double)Z;
        const double sinc = d == 0 ? 1.0 : std::sin(pi * xr) / (pi * xr);
        const double a = 1.0 - u * u;
        return (float)(s * (rolloff * sinc * spd::bessel_i0(beta * std::sqrt(a > 0.0 ? a : 0.0)) / i0b));
    };
    for (int64_t m = 0; m < q; ++m)
        for (int64_t k = 0; k < K; ++k) {
            b->w[(size_t)(m * 2 * K + k)] = weight(m + k * q);
            b->w[(size_t)(m * 2 * K + K + k)] = weight(q - m + k * q);
        }
    *out = b;
    return KWS_OK;
}

void kws_rate_bank_destroy(kws_rate_bank *bank)
{
    if (!bank) return;
    for (auto &kv : bank->dev)
        if (kv.second) (void)hipFree(kv.second);
    delete bank;
}

int kws_rate_bank_info(const kws_rate_bank *bank, int *p, int *q, int *taps)
{
    if (!bank) return fail(KWS_ERR_INVALID, "null argument");
    if (p) *p = bank->p;
    if (q) *q = bank->q;
    if (taps) *taps = bank->K;
    return KWS_OK;
}

int kws_rate_bank_weights(const kws_rate_bank *bank, float *out, size_t n)
{
    if (!bank || (!out && !bank->w.empty())) return fail(KWS_ERR_INVALID, "null argument");
    if (n < bank->w.size()) return fail(KWS_ERR_INVALID, "the bank has %zu floats, room for %zu", bank->w.size(), n);
    for (size_t i = 0; i < bank->w.size(); ++i) out[i] = bank->w[i];
    return KWS_OK;
}

int kws_rate_counts(const kws_rate_bank *bank, int64_t N, int64_t *emitted, int64_t *total)
{
    if (!bank) return fail(KWS_ERR_INVALID, "null argument");
    if (N < 0 || N > kMaxN) return fail(KWS_ERR_INVALID, "a sample count of %lld is outside [0, 2^44]", (long long)N);
    const int64_t p = bank->p, q = bank->q, K = bank->K;
    if (emitted) *emitted = N <= K ? 0 : ((N - K) * q + p - 1) / p;
    if (total) *total = (N * q + p - 1) / p;
    return KWS_OK;
}

int kws_rate_convert(const kws_rate_bank *const *banks, int n_banks, const int16_t *in, int64_t in_stride, int in_rows, const int32_t *table,
                     int A, int16_t *hist, int64_t hist_stride, int hist_rows, int16_t *out_i16, float *out_f32, int64_t out_stride,
                     int out_rows, int out_width, void *stream)
{
    if (A < 0) return fail(KWS_ERR_INVALID, "bad entry count A=%d", A);
    if (!banks || n_banks < 1 || n_banks > KWS_RATE_MAX_BANKS)
        return fail(KWS_ERR_INVALID, "a launch takes 1 .. %d banks, got %d", (int)KWS_RATE_MAX_BANKS, n_banks);
    int span_cap = 1, hist_need = 0;
    for (int i = 0; i < n_banks; ++i) {
        if (!banks[i]) return fail(KWS_ERR_INVALID, "bank %d is null", i);
        if (banks[i]->K > 0) {
            span_cap = std::max(span_cap, tile_span(banks[i]->p, banks[i]->q, banks[i]->K));
            hist_need = std::max(hist_need, 2 * banks[i]->K - 1);
        }
    }
    if (in_rows < 0 || in_stride < 1 || hist_rows < 0 || out_rows < 0 || out_stride < 1 || out_width < 0 || out_width > out_stride)
        return fail(KWS_ERR_INVALID, "bad shapes in=(%d, %lld) hist_rows=%d out=(%d, %lld) out_width=%d", in_rows, (long long)in_stride,
                    hist_rows, out_rows, (long long)out_stride, out_width);
    if ((hist_rows > 0) != (hist != nullptr)) return fail(KWS_ERR_INVALID, "hist and hist_rows=%d do not agree", hist_rows);
    if (hist_rows > 0 && hist_stride < hist_need)
        return fail(KWS_ERR_INVALID, "hist_stride=%lld is less than the 2K - 1 = %d samples a stream keeps", (long long)hist_stride, hist_need);
    if ((int64_t)out_width > (int64_t)kMaxTilesY * kTile)
        return fail(KWS_ERR_UNSUPPORTED, "out_width=%d exceeds %d x %d columns per launch", out_width, kMaxTilesY, kTile);
    if (A == 0) return KWS_OK;
    if (!table || (!in && in_rows > 0) || (!out_i16 && !out_f32)) return fail(KWS_ERR_INVALID, "null argument");
    if (out_rows == 0) return fail(KWS_ERR_INVALID, "no output rows for %d entries", A);
    Banks dv{};
    for (int i = 0; i < n_banks; ++i) {
        const float *w = nullptr;
        if (int rc = device_bank(banks[i], &w)) return rc;
        dv.b[i] = BankDev{w, banks[i]->p, banks[i]->q, banks[i]->K, 0};
    }
    const unsigned tiles = (unsigned)std::max(1, (out_width + kTile - 1) / kTile);
    const size_t smem = sizeof(float) * ((size_t)span_cap + kLdsBankFloats);
    KWS_LAUNCH("rate_convert_kernel", rate_convert_kernel, dim3((unsigned)A, tiles), dim3(kThreads), smem, static_cast<hipStream_t>(stream), dv,
               n_banks, reinterpret_cast<const short *>(in), (long)in_stride, in_rows, table, reinterpret_cast<short *>(hist),
               (long)hist_stride, hist_rows, reinterpret_cast<short *>(out_i16), out_f32, (long)out_stride, out_rows, out_width, span_cap);
    KWS_LAUNCH_CHECK("rate_convert_kernel");
    return KWS_OK;
}

}  // extern "C"
