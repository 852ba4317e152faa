// csrc/kws_reverb.hip -- RIR bank and the apply kernel of the room-reverberation augmentation (include/kws.h: kws_rir_bank_*,
// kws_reverb_apply; the convolution of tools/audio_process/audio_reverberation.py / gpuRIR_reverberation.py of the reference).
//
// One 1024-thread block per clip.  A wet clip is an FFT convolution: the clip, zero-padded to N = 32768 real samples, is packed as
// M = 16384 complex points z[n] = v[2n] + i v[2n+1]; a Stockham FFT of M points runs in four passes (radix 16, 16, 16, 4) with the 16
// points of every thread in registers and LDS used only for the exchanges between passes; the last forward pass gives every thread the
// bins k and M - k together, so the real-FFT unpacking, the product with the bank spectrum and the repacking for the inverse real FFT
// are done in registers; the inverse transform is the forward one on conjugated data.  An exchange moves the real parts and then the
// imaginary parts through one 68 KiB plane (padded every 16 floats against bank conflicts), so two blocks' worth of LDS is never held:
// what the co-running train step needs stays free.  Sums are fp32 per thread and fp64 across the block in a fixed order (no atomics),
// so two calls give the same bits.
//
// A clip of at most kDirect samples does not go through the transform.  Its output samples are few products, so |y| comes close to
// ||v|| ||h|| (for one sample they are equal), and the last bit that the float32 sums of the inverse transform lose is then as large
// as the error the tests allow (1e-7 ||v|| ||h||, less than one float32 ulp of such a y).  That clip is convolved with the bank's taps
// directly in fp64, rescaled in fp64 and rounded once.  Past a wave's worth of samples |y| / (||v|| ||h||) of a noise-like clip is
// below 3 / sqrt(64) and the transform's ulp no longer shows.
#include <cfloat>
#include <cmath>
#include <complex>
#include <vector>

#include "kws_common.h"
#include "kws_wave_stage.h"
#include "kws_device.h"
#include "kws_reverb.h"

namespace kws {
namespace rv {

constexpr int kThreads = 1024;
constexpr int kDirect = 64;                             // clips up to this many samples are convolved directly
constexpr int kPlane = M + M / 16;                      // floats of the padded exchange plane
constexpr int kLdsBytes = kPlane * (int)sizeof(float);  // 69632
enum { kRevApply = 0, kRevRir = 1, kRevFields = 2 };    // draw fields: aug_hash(seed_r, step, 2 p + f)

__device__ __forceinline__ int pad(int p) { return p + (p >> 4); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)

// forward 4-point DFT in place
__device__ __forceinline__ void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = csub(a1, a3);
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = make_float2(t1.x + t3.y, t1.y - t3.x);   // t1 - i t3
    a3 = make_float2(t1.x - t3.y, t1.y + t3.x);   // t1 + i t3
}

// forward 16-point DFT as 4 x 4: on return bin q sits in a[4 (q % 4) + q / 4] (out16 reads it in natural order)
__device__ __forceinline__ void dft16(float2 (&a)[16])
{
    constexpr float c1 = 0.923879532511286756f, s1 = 0.382683432365089772f, r2 = 0.707106781186547524f;
#pragma unroll
    for (int r0 = 0; r0 < 4; ++r0) dft4(a[r0], a[r0 + 4], a[r0 + 8], a[r0 + 12]);
    // b[r0][q0] = a[r0 + 4 q0] times exp(-2 pi i r0 q0 / 16)
    a[5] = cmul(a[5], make_float2(c1, -s1));
    a[6] = cmul(a[6], make_float2(r2, -r2));
    a[7] = cmul(a[7], make_float2(s1, -c1));
    a[9] = cmul(a[9], make_float2(r2, -r2));
    a[10] = make_float2(a[10].y, -a[10].x);
    a[11] = cmul(a[11], make_float2(-r2, -r2));
    a[13] = cmul(a[13], make_float2(s1, -c1));
    a[14] = cmul(a[14], make_float2(-r2, -r2));
    a[15] = cmul(a[15], make_float2(-c1, s1));
#pragma unroll
    for (int q0 = 0; q0 < 4; ++q0) dft4(a[4 * q0], a[4 * q0 + 1], a[4 * q0 + 2], a[4 * q0 + 3]);
}
__device__ __forceinline__ int out16(int q) { return 4 * (q & 3) + (q >> 2); }

// Move 16 values per thread through the LDS plane: value i is written at padded index wa(i) and value i read back from ra(i) (real parts,
// then imaginary parts).  Every address pattern here is a per-thread base plus a constant per i, which the LDS instructions take as their
// immediate offset.  Starts with a barrier (the plane may still be read by the previous exchange).
template <typename WA, typename RA>
__device__ __forceinline__ void exchange(float *lds, float2 (&a)[16], WA wa, RA ra)
{
    float re[16];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[wa(i)] = a[i].x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) re[i] = lds[ra(i)];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[wa(i)] = a[i].y;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = make_float2(re[i], lds[ra(i)]);
}

// exp(-2 pi i m / M) from the N-point table
__device__ __forceinline__ float2 twm(const float2 *__restrict__ tw, int m) { return tw[2 * m]; }

// The four butterflies of the last (radix-4) pass a thread owns: j and 4096 - j come in pairs, so that bins k and M - k land in the same
// thread (thread 0: 0, 2048, 1024, 3072).  Register slot s * 4 + q then holds bin jj[s] + 4096 q; bin M - k is in slot (s ^ 1) * 4 + 3 - q (thread 0: see
// reverb_apply_kernel).
__device__ __forceinline__ void last_pass_slots(int tid, int (&jj)[4])
{
    jj[0] = tid;
    jj[1] = tid ? 4096 - tid : 2048;
    jj[2] = tid ? 2048 - tid : 1024;
    jj[3] = tid ? 2048 + tid : 3072;
}

// The complex M-point FFT of the values the thread holds in the first pass's layout (a[r] = x[tid + 1024 r]).  Passes 1-3 (radix 16)
// end in an exchange into the next pass's layout; pass 4 (radix 4) leaves bin jj[s] + 4096 q in a[4 s + q].
__device__ __forceinline__ void fft_m(float *lds, float2 (&a)[16], const float2 *__restrict__ tw, int tid, const int (&jj)[4])
{
    // padded addresses: pad(b + c) = pad(b) + c + c / 16 whenever c is a multiple of 16 or b % 16 + c < 16
    const int rb = pad(tid);
    const int pj[4] = {pad(jj[0]), pad(jj[1]), pad(jj[2]), pad(jj[3])};
    auto read16 = [rb](int r) { return rb + 1088 * r; };                       // x[tid + 1024 r]
    auto read4 = [&pj](int i) { return pj[i >> 2] + 4352 * (i & 3); };         // x[jj[s] + 4096 r], i = 4 s + r
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int lg = 4 * pass, Ns = 1 << lg;                  // Ns = 1, 16, 256
        const int k = tid & (Ns - 1);
        if (pass > 0) {
            const int step = k * (M >> (lg + 4));               // exp(-2 pi i r k / (16 Ns))
#pragma unroll
            for (int r = 1; r < 16; ++r) a[r] = cmul(a[r], twm(tw, r * step));
        }
        dft16(a);
        float2 o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = a[out16(q)];
        const int wb = pad(((tid >> lg) << (lg + 4)) + k);     // output q at wb + q Ns (+ q Ns / 16)
        const int ws = Ns + (Ns >> 4);
        auto write = [wb, ws](int q) { return wb + q * ws; };
        if (pass < 2) exchange(lds, o, write, read16);
        else exchange(lds, o, write, read4);
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = o[i];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int r = 1; r < 4; ++r) a[4 * s + r] = cmul(a[4 * s + r], twm(tw, r * jj[s]));
        dft4(a[4 * s], a[4 * s + 1], a[4 * s + 2], a[4 * s + 3]);
    }
}

// Bin k of the product spectrum, repacked for the inverse real FFT (times 4, the bank spectrum carries the 1 / (4 M)): A = Z[k],
// B = Z[(M - k) mod M], Hk = H[k], Hmk = H[M - k], w = exp(-2 pi i k / N).
//   X[k] = E + w O, X[k + M] = E - w O, E = (A + conj B) / 2, O = (A - conj B) / 2i      (unpacking of the real FFT)
//   Y[k] = X[k] H[k], Y[k + M] = X[k + M] conj(H[M - k])                                 (H of a real h is Hermitian)
//   Z'[k] = (Y[k] + Y[k + M]) / 2 + i conj(w) (Y[k] - Y[k + M]) / 2                     (packing for the inverse)
__device__ __forceinline__ float2 spec_bin(float2 A, float2 B, float2 Hk, float2 Hmk, float2 w)
{
    const float2 bc = make_float2(B.x, -B.y);
    const float2 e2 = cadd(A, bc), d = csub(A, bc);
    const float2 o2 = make_float2(d.y, -d.x);
    const float2 wo = cmul(w, o2);
    const float2 P = cmul(cadd(e2, wo), Hk), Q = cmulc(csub(e2, wo), Hmk);
    const float2 ep = cadd(P, Q), op = cmulc(csub(P, Q), w);
    return make_float2(ep.x - op.y, ep.y + op.x);
}

// one pair of bins (slots i, p hold k and M - k); self pairs (k = 0, M / 2) have i == p
__device__ __forceinline__ void spec_pair(float2 (&a)[16], int i, int p, int ki, const float2 *__restrict__ H, const float2 *__restrict__ tw)
{
    const int kp = (M - ki) & (M - 1);
    const float2 Hi = H[ki], Hp = H[M - ki];
    const float2 zi = spec_bin(a[i], a[p], Hi, Hp, tw[ki]);
    if (i != p) a[p] = spec_bin(a[p], a[i], Hp, H[M - kp], tw[kp]);
    a[i] = zi;
}

__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    return s;
}

// The wet clip of lv <= kDirect samples: y[t] = sum_j v[j] h[t - j] in fp64 with the taps h[0, lh), the rescale in fp64, one rounding
// to float32.  Every thread of the block calls it; dst[0, out_stride) is written whole.
template <typename WavT>
__device__ __forceinline__ void direct_clip(const WavT *__restrict__ v, int lv, const float *__restrict__ h, int lh, int len_out,
                                            int rescale, float *__restrict__ dst, int64_t out_stride, double *red)
{
    const int tid = threadIdx.x;
    auto y_at = [&](int t) -> double {
        double acc = 0.0;
        const int j0 = t - (lh - 1) > 0 ? t - (lh - 1) : 0, j1 = t < lv - 1 ? t : lv - 1;
        for (int j = j0; j <= j1; ++j) acc = fma((double)aug_to_f32(v[j]), (double)h[t - j], acc);
        return acc;
    };
    double scale = 1.0;
    if (rescale) {
        double ev = 0.0, ey = 0.0;
        for (int j = 0; j < lv; ++j) {
            const double x = (double)aug_to_f32(v[j]);
            ev = fma(x, x, ev);
        }
        if (tid < lv && tid < len_out) {
            const double y = y_at(tid);
            ey = y * y;
        }
        const double Ey = block_sum(ey, red);
        scale = sqrt(ev / (Ey + (double)lv * (double)FLT_EPSILON));
    }
    for (int t = tid; t < len_out; t += kThreads) dst[t] = (float)(y_at(t) * scale);
    for (int64_t t = (int64_t)len_out + tid; t < out_stride; t += kThreads) dst[t] = 0.f;
}

template <typename WavT>
__global__ __launch_bounds__(1024) void reverb_apply_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ index,
                                                            const int32_t *__restrict__ valid_len, kws_reverb_params p, int K,
                                                            const int32_t *__restrict__ rir_len, const float *__restrict__ taps,
                                                            int tap_stride, const float2 *__restrict__ spec,
                                                            const float2 *__restrict__ tw, int64_t position_base, uint32_t step,
                                                            int explicit_rir, float *__restrict__ out, int64_t out_stride,
                                                            int32_t *__restrict__ lengths, int32_t *__restrict__ rir_used)
{
    extern __shared__ float lds[];
    __shared__ double red[2][kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ms = p.max_samples;
    const ClipSrc src = clip_src(index, valid_len, stride, ms, b);
    const int lv = src.clipped;

    // the host's choices are staged in `lengths` by kws_reverb_apply
    const int k = explicit_rir ? lengths[b] : aug_pick(p.seed, step, aug_pos(position_base, b, kRevFields), kRevApply, kRevRir, p.reverb_rate, K);
    const WavT *v = wav + (int64_t)src.row * stride;
    float *dst = out + (int64_t)b * out_stride;
    const int len_out = k < 0 ? lv : (lv == 0 ? 0 : (lv + rir_len[k] - 1 < ms ? lv + rir_len[k] - 1 : ms));
    __syncthreads();                                        // every thread has read lengths[b] before thread 0 overwrites it
    if (tid == 0) {
        lengths[b] = len_out;
        if (rir_used) rir_used[b] = k;
    }
    if (k < 0 || lv == 0) {                                 // dry (or empty): a copy
        dry_copy<kThreads>(dst, v, lv, out_stride);
        return;
    }
    if (lv <= kDirect) {                                    // a few samples: directly, in fp64
        direct_clip(v, lv, taps + (int64_t)k * tap_stride, rir_len[k], len_out, p.rescale, dst, out_stride, red[0]);
        return;
    }
    for (int64_t t = (int64_t)ms + tid; t < out_stride; t += kThreads) dst[t] = 0.f;

    // z[n] = v[2n] + i v[2n+1], n = tid + 1024 r; n < lv / 2 <= 8192, so r < 8 (the upper half of the input is zero: pruned loads)
    float2 a[16];
    float ev = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = 2 * (tid + 1024 * r);
        float x0 = 0.f, x1 = 0.f;
        if (r < 8) {
            if (t < lv) x0 = aug_to_f32(v[t]);
            if (t + 1 < lv) x1 = aug_to_f32(v[t + 1]);
        }
        ev = fmaf(x0, x0, ev);
        ev = fmaf(x1, x1, ev);
        a[r] = make_float2(x0, x1);
    }
    int jj[4];
    last_pass_slots(tid, jj);
    fft_m(lds, a, tw, tid, jj);

    const float2 *H = spec + (int64_t)k * kSpecStride;
    if (tid) {
#pragma unroll
        for (int r = 0; r < 4; ++r) spec_pair(a, r, 4 + 3 - r, jj[0] + 4096 * r, H, tw);
    } else {
        spec_pair(a, 0, 0, 0, H, tw);
        spec_pair(a, 1, 3, 4096, H, tw);
        spec_pair(a, 2, 2, 8192, H, tw);
        spec_pair(a, 4, 7, 2048, H, tw);
        spec_pair(a, 5, 6, 2048 + 4096, H, tw);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) spec_pair(a, 8 + r, 12 + 3 - r, jj[2] + 4096 * r, H, tw);

    // inverse: z' = conj(FFT(conj Z')); Z' goes to the plane in natural order, conjugated
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i].y = -a[i].y;
    {
        const int rb = pad(tid);
        const int pj[4] = {pad(jj[0]), pad(jj[1]), pad(jj[2]), pad(jj[3])};
        exchange(lds, a, [&pj](int i) { return pj[i >> 2] + 4352 * (i & 3); }, [rb](int r) { return rb + 1088 * r; });
    }
    // The inverse uses the forward transform's twiddles and addresses again: hide that from the compiler, which would otherwise keep
    // every twiddle offset of the forward transform live across the spectrum step (and spill).
    int tid_inv = tid;
    asm volatile("" : "+v"(tid_inv));
    last_pass_slots(tid_inv, jj);
    fft_m(lds, a, tw, tid_inv, jj);

    // y[2n] = Re, y[2n+1] = -Im at n = jj[s] + 4096 q; only n < 8192 (q < 2) can be below max_samples / 2 (pruned outputs)
    const double Ev = block_sum((double)ev, red[0]);
    float ey = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = 2 * (jj[s] + 4096 * q);
            const float y0 = a[4 * s + q].x, y1 = -a[4 * s + q].y;
            if (t < lv) ey = fmaf(y0, y0, ey);
            if (t + 1 < lv) ey = fmaf(y1, y1, ey);
        }
    float scale = 1.f;
    if (p.rescale) {
        const double Ey = block_sum((double)ey, red[1]);
        scale = (float)sqrt(Ev / (Ey + (double)lv * (double)FLT_EPSILON));
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = 2 * (jj[s] + 4096 * q);
            if (t < ms) dst[t] = t < len_out ? a[4 * s + q].x * scale : 0.f;
            if (t + 1 < ms) dst[t + 1] = t + 1 < len_out ? -a[4 * s + q].y * scale : 0.f;
        }
}

// fp64 radix-2 FFT (host, bank creation only)
void host_fft(std::vector<std::complex<double>> &x)
{
    const int n = (int)x.size();
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(x[i], x[j]);
    }
    std::vector<std::complex<double>> w(n / 2);
    for (int i = 0; i < n / 2; ++i) w[i] = std::polar(1.0, -2.0 * M_PI * i / n);
    for (int len = 2; len <= n; len <<= 1) {
        const int st = n / len;
        for (int i = 0; i < n; i += len)
            for (int j = 0; j < len / 2; ++j) {
                const std::complex<double> u = x[i + j], t = x[i + j + len / 2] * w[j * st];
                x[i + j] = u + t;
                x[i + j + len / 2] = u - t;
            }
    }
}

}  // namespace rv
}  // namespace kws

using namespace kws;
using namespace kws::rv;

extern "C" {

int kws_rir_bank_create(const float *taps, const int32_t *rir_len, int K, int max_samples, kws_rir_bank **out)
{
    if (!out || !taps || !rir_len) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (K < 1) return fail(KWS_ERR_INVALID, "a RIR bank needs at least one RIR");
    if (max_samples < 1) return fail(KWS_ERR_INVALID, "max_samples must be >= 1, got %d", max_samples);
    if (max_samples > kMaxSamples) return fail(KWS_ERR_UNSUPPORTED, "max_samples %d > %d (one %d-point transform)", max_samples, kMaxSamples, N);
    int64_t total = 0;
    for (int k = 0; k < K; ++k) {
        if (rir_len[k] < 1) return fail(KWS_ERR_INVALID, "RIR %d is empty", k);
        total += rir_len[k];
    }
    for (int64_t i = 0; i < total; ++i)
        if (!std::isfinite(taps[i])) return fail(KWS_ERR_INVALID, "RIR tap %lld is not finite", (long long)i);
    auto *rb = new kws_rir_bank();
    rb->K = K;
    rb->max_samples = max_samples;
    rb->len.resize(K);
    std::vector<float2> spec((size_t)K * kSpecStride, make_float2(0.f, 0.f));
    std::vector<float> kept((size_t)K * max_samples, 0.f);
    std::vector<std::complex<double>> x(N);
    const double norm = 1.0 / (4.0 * M);
    int64_t off = 0;
    for (int k = 0; k < K; ++k) {
        const int lh = rir_len[k] < max_samples ? rir_len[k] : max_samples;
        rb->len[k] = lh;
        std::fill(x.begin(), x.end(), std::complex<double>(0.0, 0.0));
        for (int j = 0; j < lh; ++j) x[j] = (double)taps[off + j];
        for (int j = 0; j < lh; ++j) kept[(size_t)k * max_samples + j] = taps[off + j];
        host_fft(x);
        for (int i = 0; i <= M; ++i) spec[(size_t)k * kSpecStride + i] = make_float2((float)(x[i].real() * norm), (float)(x[i].imag() * norm));
        off += rir_len[k];
    }
    std::vector<float2> tw(N);
    for (int i = 0; i < N; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / N), (float)-std::sin(2.0 * M_PI * i / N));
    auto cleanup = [&](int rc) {
        kws_rir_bank_destroy(rb);
        return rc;
    };
    if (hipMalloc(&rb->spec, sizeof(float2) * spec.size()) != hipSuccess || hipMalloc(&rb->tw, sizeof(float2) * N) != hipSuccess ||
        hipMalloc(&rb->taps, sizeof(float) * kept.size()) != hipSuccess ||
        hipMalloc(&rb->d_len, sizeof(int32_t) * K) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "RIR bank: device allocation for %d spectra failed", K));
    }
    if (hipMemcpy(rb->spec, spec.data(), sizeof(float2) * spec.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rb->tw, tw.data(), sizeof(float2) * N, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rb->taps, kept.data(), sizeof(float) * kept.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rb->d_len, rb->len.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return cleanup(fail(KWS_ERR_HIP, "RIR bank: upload failed"));
    }
    *out = rb;
    return KWS_OK;
}

void kws_rir_bank_destroy(kws_rir_bank *rb)
{
    if (!rb) return;
    if (rb->spec) (void)hipFree(rb->spec);
    if (rb->tw) (void)hipFree(rb->tw);
    if (rb->taps) (void)hipFree(rb->taps);
    if (rb->d_len) (void)hipFree(rb->d_len);
    delete rb;
}

int kws_rir_bank_info(const kws_rir_bank *rb, int *K, int *max_samples, int *fft_size)
{
    if (!rb) return fail(KWS_ERR_INVALID, "null argument");
    if (K) *K = rb->K;
    if (max_samples) *max_samples = rb->max_samples;
    if (fft_size) *fft_size = N;
    return KWS_OK;
}

int kws_reverb_apply(const kws_rir_bank *rb, const kws_reverb_params *p, const void *wav, int wav_dtype, const int32_t *index, int B,
                     int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const int32_t *explicit_rir, float *out,
                     int64_t out_stride, int32_t *lengths, int32_t *rir_used, void *stream)
{
    if (!rb || !p || (B > 0 && (!wav || !out || !lengths))) return fail(KWS_ERR_INVALID, "null argument");
    if (rb->K < 1) return fail(KWS_ERR_INVALID, "empty RIR bank");
    if (!(p->reverb_rate >= 0.f && p->reverb_rate <= 1.f)) return fail(KWS_ERR_INVALID, "reverb_rate %g is outside [0, 1]", (double)p->reverb_rate);
    if (int rc = check_clip_batch(p->max_samples, kMaxSamples, B, stride, false, valid_len, position_base, &out_stride, wav_dtype)) return rc;
    if (explicit_rir)
        for (int b = 0; b < B; ++b)
            if (explicit_rir[b] < -1 || explicit_rir[b] >= rb->K)
                return fail(KWS_ERR_INVALID, "clip %d: RIR %d is outside [-1, %d)", b, explicit_rir[b], rb->K);
    if (B == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (explicit_rir) KWS_HIP_CHECK(hipMemcpyAsync(lengths, explicit_rir, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)B), block(kThreads);
    return for_wav_type(wav_dtype, "reverb_apply_f32", "reverb_apply_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(reverb_apply_kernel<WavT>), kLdsBytes)) return rc;
        KWS_LAUNCH(name, reverb_apply_kernel<WavT>, grid, block, kLdsBytes, s, static_cast<const WavT *>(wav), stride, index, valid_len, *p,
                   rb->K, rb->d_len, rb->taps, rb->max_samples, rb->spec, rb->tw, position_base, (uint32_t)step, explicit_rir ? 1 : 0, out, out_stride, lengths, rir_used);
        KWS_LAUNCH_CHECK("reverb_apply_kernel");
        return KWS_OK;
    });
}

}  // extern "C"
