// csrc/kws_synth.hip -- labelled streaming test recordings from clips (include/kws.h): the placement kernel (one wave per recording),
// the gain kernel (one wave per placed slot) and the render kernel (one block per tile of a recording).  The noise bank and its fp64
// prefix sums are kws_augment.hip's; the draws and the sample conversion are kws_wave_stage.h's.
#include <cfloat>
#include <climits>
#include <cmath>

#include "kws_common.h"
#include "kws_augment.h"
#include "kws_device.h"

namespace kws {

constexpr int kSynthTile = 4096;      // samples of a recording per render block
constexpr int kSynthThreads = 256;
constexpr int kSynthStage = 256;      // events of a tile kept in LDS; a tile that meets more reads the rest from global memory

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ long long wave_scan(long long v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// One wave per recording: the bed's draws, then the slots in groups of 64 (lane = slot within the group).  end_j = lead_in + sum_{i<=j}
// (len_i + gap_i) never decreases with j, so the slots that fit are the leading ones; `open` turns false at the first that does not.
__global__ __launch_bounds__(256) void synth_place_kernel(int rows, int64_t stride, const int32_t *__restrict__ valid_len,
                                                          const int32_t *__restrict__ pick, int M, const int32_t *__restrict__ lengths, int R,
                                                          int max_events, kws_synth_params p, int K, const int32_t *__restrict__ seg_len,
                                                          int64_t position_base, kws_synth_rec *__restrict__ rec,
                                                          kws_synth_event *__restrict__ events)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= R) return;
    const uint32_t pos = (uint32_t)(position_base + r);
    const long long N = lengths[r] > 0 ? lengths[r] : 0;
    kws_synth_rec rc = {-1, 0, 0.f, 0};
    if (K > 0) {
        rc.segment = (int)aug_uniform(aug_hash(p.seed, pos, 0), (uint32_t)K);
        rc.offset = (int)aug_uniform(aug_hash(p.seed, pos, 1), (uint32_t)seg_len[rc.segment]);
        rc.bed_gain = fmaf(aug_unit(aug_hash(p.seed, pos, 2)), p.bed_gain_hi - p.bed_gain_lo, p.bed_gain_lo);
    }
    long long carry = p.lead_in;
    bool open = true;
    int n_events = 0;
    kws_synth_event *ev = events + (int64_t)r * max_events;
    for (int base = 0; base < max_events; base += 64) {
        const int j = base + lane;
        const bool active = j < max_events;
        int row = -1, len = 0, gap = 0;
        float snr = 0.f;
        if (active) {
            const uint32_t f = 4u + 3u * (uint32_t)j;
            const int sel = (int)aug_uniform(aug_hash(p.seed, pos, f), (uint32_t)M);
            row = pick ? pick[sel] : sel;
            gap = p.gap_lo + (int)aug_uniform(aug_hash(p.seed, pos, f + 1), (uint32_t)(p.gap_hi - p.gap_lo) + 1u);
            if (p.n_snr > 0) snr = p.snr_db[aug_uniform(aug_hash(p.seed, pos, f + 2), (uint32_t)p.n_snr)];
            if (row >= 0 && row < rows) {           // a pick outside the store places an empty clip
                int64_t l = valid_len ? (int64_t)valid_len[row] : stride;
                l = l < 0 ? 0 : l > stride ? stride : l;
                len = l < p.clip_cap ? (int)l : p.clip_cap;
            }
        }
        const long long end = carry + wave_scan(active ? (long long)len + gap : 0ll, lane);
        const bool fit = active && end <= N;
        const unsigned long long miss = ~__ballot(fit);
        const int first_miss = miss ? __ffsll((long long)miss) - 1 : 64;
        const bool placed = open && lane < first_miss;
        if (active) {
            kws_synth_event e = {-1, 0, 0, 0.f, 0.f, {0, 0, 0}};
            if (placed) {
                e.row = row;
                e.start = (int)(end - len);
                e.length = len;
                e.snr_db = snr;
                e.gain = len > 0 ? 1.f : 0.f;       // synth_gain_kernel replaces it when there is an SNR and a bed
            }
            ev[j] = e;
        }
        if (open) n_events += first_miss;
        if (first_miss < 64) open = false;
        carry = __shfl(end, 63, 64);
    }
    rc.n_events = n_events;
    if (lane == 0) rec[r] = rc;
}

// sum of prefix[a .. a + n) of a segment of L samples read circularly from a in [0, L): whole loops plus at most two pieces
__device__ __forceinline__ double circular_power(const double *__restrict__ P, int L, int a, int n)
{
    const int n1 = n < L - a ? n : L - a;
    double s = P[a + n1] - P[a];
    const int rem = n - n1;
    if (rem > 0) {
        s += (double)(rem / L) * (P[L] - P[0]);
        s += P[rem % L] - P[0];
    }
    return s;
}

// One wave per slot (r, j) of the placed plan: the gain of include/kws.h.  Lanes stride over the clip with fp32 partials (the noise
// plan's order, kws_augment.hip), one fp64 wave sum.
template <typename WavT>
__global__ __launch_bounds__(256) void synth_gain_kernel(const WavT *__restrict__ wav, int rows, int64_t stride, int R, int max_events,
                                                         float max_gain, const int32_t *__restrict__ seg_len, const double *__restrict__ prefix,
                                                         const int64_t *__restrict__ seg_start, const kws_synth_rec *__restrict__ rec,
                                                         kws_synth_event *__restrict__ events)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (slot >= (int64_t)R * max_events) return;
    const int r = (int)(slot / max_events);
    const kws_synth_event e = events[slot];
    if (e.row < 0 || e.row >= rows || e.length <= 0) return;
    const kws_synth_rec rc = rec[r];
    const int L = e.length;
    const WavT *v = wav + (int64_t)e.row * stride;
    float part = 0.f;
    for (int t = lane; t < L; t += 64) {
        const float x = aug_to_f32(v[t]);
        part = fmaf(x, x, part);
    }
    const double pv = wave_sum((double)part) / L;
    const int Lk = seg_len[rc.segment];
    const int a = (int)(((uint32_t)rc.offset + (uint32_t)e.start) % (uint32_t)Lk);
    const double pn = (double)rc.bed_gain * (double)rc.bed_gain * (circular_power(prefix + seg_start[rc.segment], Lk, a, L) / L);
    const float g = (float)sqrt(pow(10.0, (double)e.snr_db / 10.0) * pn / (pv + (double)FLT_EPSILON));
    if (lane == 0) events[slot].gain = g < max_gain ? g : max_gain;
}

__device__ __forceinline__ void synth_store(float *dst, float x) { *dst = x; }
__device__ __forceinline__ void synth_store(short *dst, float x)
{
    const float y = rintf(__fmul_rn(x, 32768.f));
    *dst = (short)(y < -32768.f ? -32768.f : y > 32767.f ? 32767.f : y);
}

// One block per tile of kSynthTile samples of one recording.  The block finds [e0, e1), the events that meet the tile, by binary search over the sorted slots and stages them in
// LDS as {start, end, row, gain}.  The samples are computed one per lane into LDS (every global load coalesced: first the bed, then
// the staged events one after the other) and leave it V at a time, one 128-bit store per thread when VEC.
template <typename WavT, typename OutT, bool VEC>
__global__ __launch_bounds__(kSynthThreads) void synth_render_kernel(const WavT *__restrict__ wav, int rows, int64_t stride,
                                                                     const kws_synth_rec *__restrict__ rec,
                                                                     const kws_synth_event *__restrict__ events, int max_events,
                                                                     const int32_t *__restrict__ lengths, int max_len, float inv_fade, int K,
                                                                     const float *__restrict__ bank, const int64_t *__restrict__ seg_start,
                                                                     const int32_t *__restrict__ seg_len, OutT *__restrict__ out, int64_t out_stride)
{
    constexpr int V = 16 / (int)sizeof(OutT);
    __shared__ int4 staged[kSynthStage];
    __shared__ float tile[kSynthTile] __attribute__((aligned(16)));
    const int r = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kSynthTile;
    const int64_t t1 = t0 + kSynthTile < out_stride ? t0 + kSynthTile : out_stride;
    int N = lengths[r];
    N = N < 0 ? 0 : N > max_len ? max_len : N;
    OutT *dst = out + (int64_t)r * out_stride;
    const kws_synth_rec rc = rec[r];
    const kws_synth_event *ev = events + (int64_t)r * max_events;
    const int n_ev = rc.n_events < 0 ? 0 : rc.n_events > max_events ? max_events : rc.n_events;

    int e0 = 0, e1 = 0;                              // the same loads in every lane
    if (t0 < N) {
        int lo = 0, hi = n_ev;                       // first event that ends after t0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)ev[mid].start + ev[mid].length > t0) hi = mid; else lo = mid + 1;
        }
        e0 = lo;
        hi = n_ev;                                   // first event that starts at or after t1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ev[mid].start >= t1) hi = mid; else lo = mid + 1;
        }
        e1 = lo;
    }
    const int cnt = e1 - e0;
    // {start, end, row, gain} of event e0 + i; an unusable slot becomes empty (end = start)
    auto load_event = [&](int i) {
        const kws_synth_event e = ev[e0 + i];
        const bool ok = e.row >= 0 && e.row < rows && e.length > 0 && e.start >= 0;
        const int64_t len = ok ? (e.length < stride ? (int64_t)e.length : stride) : 0;
        const int64_t end = (int64_t)e.start + len < N ? (int64_t)e.start + len : N;
        return make_int4(e.start, end > e.start ? (int)end : e.start, e.row, __float_as_int(e.gain));
    };
    for (int i = tid; i < cnt && i < kSynthStage; i += kSynthThreads) staged[i] = load_event(i);
    __syncthreads();
    auto event_at = [&](int i) { return i < kSynthStage ? staged[i] : load_event(i); };

    const bool bed = K > 0 && rc.segment >= 0 && rc.segment < K;
    const uint32_t Lk = bed ? (uint32_t)seg_len[rc.segment] : 1u;
    const float *nk = bed ? bank + seg_start[rc.segment] : nullptr;
    // o < Lk <= INT_MAX and t0 < N <= INT_MAX: the sum fits 32 bits
    const uint32_t pos0 = bed && t0 < N ? ((uint32_t)rc.offset % Lk + (uint32_t)t0) % Lk : 0u;
    const int tile_len = (int)(t1 - t0);

    // Phase 1, lane = sample: sample t0 + j belongs to thread j mod kSynthThreads in both passes, so they need no barrier between them.
    // The bed: every load of the tile is issued before the first is used, consecutive lanes on consecutive samples.
#pragma unroll
    for (int k = 0; k < kSynthTile / kSynthThreads; ++k) {
        const int j = tid + k * kSynthThreads;
        float s = 0.f;
        if (bed && t0 + j < N) {
            uint32_t pos = pos0 + (uint32_t)j;                     // < 2 Lk for a segment of at least a tile
            if (pos >= Lk) pos = Lk >= (uint32_t)kSynthTile ? pos - Lk : pos % Lk;
            s = __fmul_rn(rc.bed_gain, nk[pos]);
        }
        tile[j] = s;
    }
    // The clips: event by event (the same for the whole block), the event's samples inside the tile strided over the threads.
    for (int i = 0; i < cnt; ++i) {
        const int4 e = event_at(i);
        const int ja = e.x > t0 ? (int)(e.x - t0) : 0, jb = e.y < t1 ? (int)(e.y - t0) : tile_len;
        const WavT *v = wav + (int64_t)e.z * stride;
        const float g = __int_as_float(e.w);
        const int len = e.y - e.x;
#pragma unroll 4
        for (int j = ja + ((tid - ja) & (kSynthThreads - 1)); j < jb; j += kSynthThreads) {
            const int u = (int)(t0 + j - e.x);
            const float a = __fmul_rn((float)(u + 1), inv_fade), b = __fmul_rn((float)(len - u), inv_fade);
            const float w = fminf(1.f, fminf(a, b));
            tile[j] = __fmaf_rn(__fmul_rn(g, w), aug_to_f32(v[u]), tile[j]);
        }
    }
    __syncthreads();
    // Phase 2: V consecutive samples per thread from LDS, converted, one 128-bit store; without the alignment one sample per lane
    if (VEC) {
        for (int j = tid * V; j < tile_len; j += kSynthThreads * V) {
            OutT y[V] __attribute__((aligned(16)));
#pragma unroll
            for (int q = 0; q < V; ++q) synth_store(&y[q], tile[j + q]);
            *reinterpret_cast<int4 *>(dst + t0 + j) = *reinterpret_cast<const int4 *>(y);
        }
    } else {
        for (int j = tid; j < tile_len; j += kSynthThreads) synth_store(dst + t0 + j, tile[j]);
    }
}

static int check_synth_shape(int max_events, int fade, int R, int rows, int64_t stride, int wav_dtype)
{
    if (max_events < 1 || max_events > KWS_SYNTH_MAX_EVENTS)
        return fail(KWS_ERR_INVALID, "max_events %d is outside 1..%d", max_events, KWS_SYNTH_MAX_EVENTS);
    if (fade < 0) return fail(KWS_ERR_INVALID, "fade %d is negative", fade);
    if (R < 0 || rows < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative recordings, rows or stride");
    if (stride > INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "stride %lld does not fit 31 bits", (long long)stride);
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    return KWS_OK;
}

template <typename WavT, typename OutT>
static int synth_render_launch(const kws_noise_bank *bank, const WavT *wav, int rows, int64_t stride, const kws_synth_rec *rec,
                               const kws_synth_event *events, int max_events, const int32_t *lengths, int R, int max_len, float inv_fade,
                               OutT *out, int64_t out_stride, const char *name, hipStream_t s)
{
    const dim3 grid((unsigned)((out_stride + kSynthTile - 1) / kSynthTile), (unsigned)R), block(kSynthThreads);
    const int K = bank ? bank->K : 0;
    const float *samples = bank ? bank->samples : nullptr;
    const int64_t *d_start = bank ? bank->d_start : nullptr;
    const int32_t *d_len = bank ? bank->d_len : nullptr;
    // 128-bit stores: every row starts on 16 bytes and holds whole vectors (a tile is a multiple of both vector widths)
    const bool vec = reinterpret_cast<uintptr_t>(out) % 16 == 0 && (out_stride * (int64_t)sizeof(OutT)) % 16 == 0;
    if (vec)
        KWS_LAUNCH(name, (synth_render_kernel<WavT, OutT, true>), grid, block, 0, s, wav, rows, stride, rec, events, max_events, lengths, max_len,
                   inv_fade, K, samples, d_start, d_len, out, out_stride);
    else
        KWS_LAUNCH(name, (synth_render_kernel<WavT, OutT, false>), grid, block, 0, s, wav, rows, stride, rec, events, max_events, lengths, max_len,
                   inv_fade, K, samples, d_start, d_len, out, out_stride);
    KWS_LAUNCH_CHECK("synth_render_kernel");
    return KWS_OK;
}

}  // namespace kws

using namespace kws;

extern "C" {

int kws_synth_plan(const kws_noise_bank *bank, const kws_synth_params *params, const void *wav, int wav_dtype, int rows, int64_t stride,
                   const int32_t *valid_len, const int32_t *pick, int M, const int32_t *lengths, int R, int max_events,
                   int64_t position_base, kws_synth_rec *rec, kws_synth_event *events, void *stream)
{
    if (!params) return fail(KWS_ERR_INVALID, "null synth params");
    const kws_synth_params &p = *params;
    if (p.gap_lo < 0 || p.gap_hi < p.gap_lo) return fail(KWS_ERR_INVALID, "gaps [%d, %d] need 0 <= gap_lo <= gap_hi", p.gap_lo, p.gap_hi);
    if (p.lead_in < 0) return fail(KWS_ERR_INVALID, "lead_in %d is negative", p.lead_in);
    if (p.clip_cap < 1) return fail(KWS_ERR_INVALID, "clip_cap %d must be >= 1", p.clip_cap);
    if (p.n_snr < 0 || p.n_snr > KWS_AUG_MAX_SNR) return fail(KWS_ERR_INVALID, "the SNR list takes 0..%d entries, got %d", KWS_AUG_MAX_SNR, p.n_snr);
    for (int i = 0; i < p.n_snr; ++i)
        if (!std::isfinite(p.snr_db[i])) return fail(KWS_ERR_INVALID, "SNR %d is not finite", i);
    if (!(p.bed_gain_hi >= p.bed_gain_lo)) return fail(KWS_ERR_INVALID, "bed gains [%g, %g] need lo <= hi", (double)p.bed_gain_lo, (double)p.bed_gain_hi);
    if (!(p.max_gain > 0.f)) return fail(KWS_ERR_INVALID, "max_gain %g must be positive", (double)p.max_gain);
    if (int rc = check_synth_shape(max_events, p.fade, R, rows, stride, wav_dtype)) return rc;
    if (int rc = check_clip_batch(p.clip_cap, INT_MAX, R, stride, true, valid_len, position_base, nullptr, wav_dtype)) return rc;
    if (R == 0) return KWS_OK;
    if (rows < 1 || M < 1 || (!pick && M != rows)) return fail(KWS_ERR_INVALID, "the clip store and the pick table need at least one row (M = rows without a table)");
    if (!wav || !lengths || !rec || !events) return fail(KWS_ERR_INVALID, "null argument");
    if (bank && bank->K < 1) return fail(KWS_ERR_INVALID, "empty noise bank");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = bank ? bank->K : 0;
    const int with_gain = K > 0 && p.n_snr > 0;
    KWS_LAUNCH("synth_place", synth_place_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, rows, stride, valid_len, pick, M, lengths, R,
               max_events, p, K, bank ? bank->d_len : nullptr, position_base, rec, events);
    KWS_LAUNCH_CHECK("synth_place_kernel");
    if (!with_gain) return KWS_OK;
    const dim3 grid((unsigned)(((int64_t)R * max_events + 3) / 4)), block(256);
    return for_wav_type(wav_dtype, "synth_gain_f32", "synth_gain_i16", [&](auto t, const char *name) -> int {
        using WavT = decltype(t);
        KWS_LAUNCH(name, synth_gain_kernel<WavT>, grid, block, 0, s, static_cast<const WavT *>(wav), rows, stride, R, max_events, p.max_gain,
                   bank->d_len, bank->prefix, bank->d_start, rec, events);
        KWS_LAUNCH_CHECK("synth_gain_kernel");
        return KWS_OK;
    });
}

int kws_synth_render(const kws_noise_bank *bank, const void *wav, int wav_dtype, int rows, int64_t stride, const kws_synth_rec *rec,
                     const kws_synth_event *events, int max_events, const int32_t *lengths, int R, int64_t max_len, int fade,
                     void *out, int out_dtype, int64_t out_stride, void *stream)
{
    if (int rc = check_synth_shape(max_events, fade, R, rows, stride, wav_dtype)) return rc;
    if (out_dtype != KWS_WAV_F32 && out_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown output dtype %d", out_dtype);
    if (max_len < 0) return fail(KWS_ERR_INVALID, "max_len %lld is negative", (long long)max_len);
    if (max_len > INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "max_len %lld does not fit 31 bits", (long long)max_len);
    if (out_stride < max_len) return fail(KWS_ERR_INVALID, "out_stride %lld < max_len %lld", (long long)out_stride, (long long)max_len);
    if (R == 0 || out_stride == 0) return KWS_OK;
    if (!rec || !events || !lengths || !out || (rows > 0 && !wav)) return fail(KWS_ERR_INVALID, "null argument");
    if (bank && bank->K < 1) return fail(KWS_ERR_INVALID, "empty noise bank");
    if ((out_stride + kSynthTile - 1) / kSynthTile > INT_MAX || R > 65535)
        return fail(KWS_ERR_UNSUPPORTED, "%d recordings of %lld samples exceed one launch (65535 recordings)", R, (long long)out_stride);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float inv_fade = 1.0f / (float)(fade + 1);
    return for_wav_type(wav_dtype, "f32", "i16", [&](auto t, const char *) -> int {
        using WavT = decltype(t);
        const WavT *w = static_cast<const WavT *>(wav);
        if (out_dtype == KWS_WAV_F32)
            return synth_render_launch(bank, w, rows, stride, rec, events, max_events, lengths, R, (int)max_len, inv_fade, static_cast<float *>(out),
                                       out_stride, wav_dtype == KWS_WAV_F32 ? "synth_render_f32_f32" : "synth_render_i16_f32", s);
        return synth_render_launch(bank, w, rows, stride, rec, events, max_events, lengths, R, (int)max_len, inv_fade, static_cast<short *>(out),
                                   out_stride, wav_dtype == KWS_WAV_F32 ? "synth_render_f32_i16" : "synth_render_i16_i16", s);
    });
}

}  // extern "C"
