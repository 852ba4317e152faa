// csrc/kws_stream.hip -- streaming post-processing for S concurrent audio streams (gfx950 only).
//
// Replaces the per-chunk Python of the reference's listen.py, batched over streams:
//   ThresholdDecoder          listen.py:452-522   -> kws_decoder_* (table built once on the host in double, kept on device)
//   TriggerDetector.update    listen.py:538-559   -> kws_trigger_update
//   update_vectors (rows)     listen.py:107-109   -> kws_stream_push_rows
//   the prediction loop       listen.py:361-375   -> kws_stream_postprocess (argmax + max + decode + trigger, one kernel)
// and the time-parallel form of the same loop over whole recordings (kws_amd.stream.scan):
//   update_vectors (windows)  listen.py:96-114    -> kws_stream_gather_windows (every chunk's feature matrix from the recording's rows)
//   the prediction loop       listen.py:361-375   -> kws_stream_scan_postprocess (argmax / max / decode per chunk in parallel, then the
//                                                    trigger walked in chunk order, one wave per recording)
//   TriggerDetector.update    listen.py:538-559   -> kws_stream_sweep (the same walk over a scan's decoded scores at 64 operating points
//                                                    per wave, one per lane, counted against labelled events)
// and the harvest of a scan for the next training run (kws_amd.stream.collect / peaks):
//   Listener.on_activation    listen.py:291-308   -> kws_stream_collect (the walk once more at one operating point, every activation
//                                                    recorded with its chunk, class and kind -- hit, duplicate, false alarm)
//   (nothing in the reference)                    -> kws_stream_peaks (the near misses: the best well-separated non-background chunks)
// and the same per-chunk loop for streams that do NOT advance together (kws_amd.stream.StreamServer):
//   update_vectors (samples)  listen.py:96-105    -> kws_stream_ragged_append (carry + chunk -> compact row, carry shifted in the same kernel)
//   update_vectors (rows)     listen.py:107-109   -> kws_stream_ragged_push_rows (each slot slides by its own row count)
//   the prediction loop       listen.py:361-375   -> kws_stream_ragged_postprocess (per-slot sensitivity, trigger level and state)
// Shared device code: the kernels that step the detector through a recording are one walk, walk_chunks, plus their own few lines
// (scan_trigger, sweep; collect keeps the loop written out, for speed); the ones that hold chunks against labelled events (sweep,
// collect, peaks) use one EventMatcher; the lockstep and the ragged sliding window are one pass, slide_window.
// Everything here is a few bytes per stream and one thread per stream: the kernels are latency-sized, the point of doing
// them on the device is that probabilities, scores and detector state never leave HBM between the forward pass of one
// chunk and the next (the whole step can sit in one hipGraph).  Arithmetic is float64 wherever the reference computes
// with Python floats, so activation decisions are identical, not just close.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kws_common.h"

struct kws_decoder {
    int32_t min_out, out_range;
    int64_t n;                 // len(cd)
    double center;
    std::vector<double> cd;    // host copy (encode, kws_decoder_table)
    double *d_cd;              // device copy
};

namespace kws {

struct DecDev {
    const double *cd;
    long n;
    int min_out, out_range;
    double center;
    int enabled;
};

// ThresholdDecoder.decode, listen.py:496-508.  `odds` is 1/x - 1 as the caller's precision produced it.
__device__ __forceinline__ double decode_one(double x, double odds, const DecDev &d)
{
    if (x == 1.0 || x == 0.0) return x;
    double cp;
    if (d.out_range == 0) {
        cp = x > (double)d.min_out ? 1.0 : 0.0;
    } else {
        const double logit = (x > 0.0 && x < 1.0) ? -log(odds) : -10.0;            // asigmoid, listen.py:480-485
        double ratio = (logit - (double)d.min_out) / (double)d.out_range;
        ratio = fmin(fmax(ratio, 0.0), 1.0);
        cp = d.cd[(long)(ratio * (double)(d.n - 1) + 0.5)];
    }
    return cp < d.center ? 0.5 * cp / d.center : 0.5 + 0.5 * (cp - d.center) / (1.0 - d.center);
}

__device__ __forceinline__ double decode_f64(double x, const DecDev &d) { return decode_one(x, 1.0 / x - 1.0, d); }
// float32 network output: numpy evaluates `1 / x - 1` in float32 (listen.py:361-367 hands decode a float32 array)
__device__ __forceinline__ double decode_f32(float x, const DecDev &d) { return decode_one((double)x, (double)(1.0f / x - 1.0f), d); }

template <typename T>
__global__ __launch_bounds__(256) void decode_kernel(const T *__restrict__ raw, double *__restrict__ out, long n, DecDev d)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (sizeof(T) == 4) out[i] = decode_f32((float)raw[i], d);
    else out[i] = decode_f64((double)raw[i], d);
}

// TriggerDetector.update, listen.py:538-559.  st = {activation, record_index}
__device__ __forceinline__ int trigger_one(int index, double score, int background, double sensitivity, int level, int refractory,
                                           int32_t *st)
{
    int act = st[0];
    const int rec = st[1];
    if (index != background && index == rec && score > sensitivity) {
        act += 1;
        if (act > level) {
            st[0] = refractory;            // -(8 * 2048) // chunk_size; record_index stays (it equals index)
            return 1;
        }
    } else if (act < 0) {
        act += 1;
    } else if (act > 0) {
        act -= 1;
    }
    st[0] = act;
    st[1] = index;
    return 0;
}

__global__ __launch_bounds__(256) void trigger_kernel(const int32_t *__restrict__ index, const double *__restrict__ score, int S,
                                                       int background, double sensitivity, int level, int refractory,
                                                       int32_t *__restrict__ state, int32_t *__restrict__ fired)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    fired[s] = trigger_one(index[s], score[s], background, sensitivity, level, refractory, state + 2 * (long)s);
}

// listen.py:361-367 for one row of probabilities: first maximum (np.argmax), np.max, decode unless background
__device__ __forceinline__ int argmax_decode(const float *__restrict__ p, int C, int background, const DecDev &d, double &score)
{
    float best = p[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = p[c];
        if (v > best) { best = v; arg = c; }
    }
    score = (double)best;
    if (arg != background && d.enabled) score = decode_f32(best, d);
    return arg;
}

// one thread per stream: first maximum (np.argmax), decode unless background, detector update
__global__ __launch_bounds__(256) void postprocess_kernel(const float *__restrict__ probs, int S, int C, int background, DecDev d,
                                                           double sensitivity, int level, int refractory,
                                                           int32_t *__restrict__ state, int32_t *__restrict__ index,
                                                           double *__restrict__ score, int32_t *__restrict__ fired)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    double sc;
    const int arg = argmax_decode(probs + (long)s * C, C, background, d, sc);
    index[s] = arg;
    score[s] = sc;
    fired[s] = trigger_one(arg, sc, background, sensitivity, level, refractory, state + 2 * (long)s);
}

// The sliding-window pass of one block of 256 threads: the window f of `total` floats moves left by `shift` and r[0 .. shift) comes
// in behind it (`reset`: zeros stand for the old window).  Every element of a pass (2048) is read into a register before the barrier,
// so the in-place shift has no hazards.  `store` writes the window back to f; kCompact writes it a second time, to o.
template <bool kCompact>
__device__ __forceinline__ void slide_window(float *__restrict__ f, const float *__restrict__ r, int total, int shift, bool reset, bool store,
                                             float *__restrict__ o)
{
    constexpr int kPer = 8;                                                          // F*D <= 2048 per pass
    for (int base = 0; base < total; base += 256 * kPer) {
        float v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = base + threadIdx.x + 256 * j;
            v[j] = 0.f;
            if (i < total) v[j] = i + shift < total ? (reset ? 0.f : f[i + shift]) : r[i + shift - total];
        }
        __syncthreads();     // the reads of this pass precede its writes; later passes only read further right
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = base + threadIdx.x + 256 * j;
            if (i < total) {
                if (store) f[i] = v[j];
                if (kCompact) o[i] = v[j];
            }
        }
        __syncthreads();
    }
}

// block = one stream
__global__ __launch_bounds__(256) void push_rows_kernel(float *__restrict__ feat, const float *__restrict__ rows, int F, int D,
                                                         int n_rows, int n_keep)
{
    const int s = blockIdx.x;
    const float *r = rows + (long)s * n_rows * D + (long)(n_rows - n_keep) * D;     // the last n_keep new rows
    slide_window<false>(feat + (long)s * F * D, r, F * D, n_keep * D, false, true, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// Offline scan of whole recordings.  With W = window, H = hop, c = chunk_size and a recording of N samples, the chunk loop
// (StreamBatch.push per chunk) has after its k-th chunk (1-based) n_k = min(k c, N) samples and -- its carry buffer always
// starts on a frame boundary -- r_k = 0 if n_k < W else (n_k - W) / H + 1 rows, row j being vectorize_raw of samples
// [j H, j H + W); the matrix the model sees is rows [r_k - F, r_k), zeros for negative indices (listen.py:92).
// Precondition: H <= W.  With H > W a push can consume more samples than the carry holds; the loop then empties the carry
// (listen.py:105) and its next frame starts with the next chunk, not on a multiple of H, so r_k depends on the chunking and
// this closed form does not hold: kws_stream_gather_windows refuses such a geometry (as kws_amd.stream.scan_plan / scan do).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long scan_rows_after(long k, int chunk, long N, int W, int H)
{
    long n = k * chunk;
    n = n < N ? n : N;
    return n < W ? 0 : (n - W) / H + 1;
}

// block = one window (recording r, chunk k0 + i): F * D consecutive floats of the recording's rows ending at row r_k
__global__ __launch_bounds__(256) void gather_windows_kernel(const float *__restrict__ rows, int max_frames, const int32_t *__restrict__ lengths,
                                                              int chunk, int W, int H, int F, int D, long k0, int n_chunks, long n_windows,
                                                              float *__restrict__ feat)
{
    const int total = F * D;
    for (long w = blockIdx.x; w < n_windows; w += gridDim.x) {
        const int r = (int)(w / n_chunks);
        const long k = k0 + (w - (long)r * n_chunks) + 1;                          // 1-based chunk number
        long N = lengths[r];
        N = N < 0 ? 0 : N;
        const long T = (N + chunk - 1) / chunk;
        long rk = k <= T ? scan_rows_after(k, chunk, N, W, H) : 0;                 // past the recording: the all-zero matrix
        rk = rk < max_frames ? rk : max_frames;
        const float *src = rows + ((long)r * max_frames + rk - F) * D;             // element e of the window is src[e] when its row exists
        const int first = rk >= F ? 0 : (int)(F - rk) * D;
        float *dst = feat + w * total;
        for (int e = threadIdx.x; e < total; e += 256) dst[e] = e >= first ? src[e] : 0.f;
    }
}

// argmax / max / decode of every (recording, chunk) of a tile; chunks at or past the recording's count get index -1, score 0
__global__ __launch_bounds__(256) void scan_decode_kernel(const float *__restrict__ probs, int n_chunks, int C, const int32_t *__restrict__ rec_chunks,
                                                          long k0, int background, DecDev d, long n_windows, long out_stride,
                                                          int32_t *__restrict__ index, double *__restrict__ score)
{
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_windows) return;
    const int r = (int)(w / n_chunks);
    const long i = w - (long)r * n_chunks;
    int arg = -1;
    double sc = 0.0;
    if (k0 + i < rec_chunks[r]) arg = argmax_decode(probs + w * C, C, background, d, sc);
    index[r * out_stride + i] = arg;
    score[r * out_stride + i] = sc;
}

// wave-uniform broadcast of lane j's value (j is the same in every lane): v_readlane into scalar registers, no LDS round trip
__device__ __forceinline__ int lane_value(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double lane_value(double v, int j)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// a chunk count read from device memory, clamped to 0 .. limit: no walk leaves its row, whatever rec_chunks holds
__device__ __forceinline__ long clamp_chunks(long T, long limit) { return T < 0 ? 0 : (T < limit ? T : limit); }

// The walk over one row of T chunks, by one wave; a kernel that steps the detector through a recording is this plus its own few
// lines (collect_kernel says why it is not).  64 chunks' (index, score) are loaded at once, one per lane, and step(k, index_k, score_k) runs once per chunk in chunk
// order with wave-uniform arguments (lane_value); after each group of up to 64 chunks, group(base) runs with the group's first chunk.
template <typename Step, typename Group>
__device__ __forceinline__ void walk_chunks(const int32_t *__restrict__ row_index, const double *__restrict__ row_score, long T, Step step,
                                            Group group)
{
    const int lane = threadIdx.x;
    for (long base = 0; base < T; base += 64) {
        const long i = base + lane;
        int idx = -1;
        double sc = 0.0;
        if (i < T) { idx = row_index[i]; sc = row_score[i]; }
        const int n = (int)(T - base < 64 ? T - base : 64);
        for (int j = 0; j < n; ++j) step((int)base + j, lane_value(idx, j), lane_value(sc, j));
        group(base);
    }
}

// block = one wave = one recording: the walk with the state in registers, the same in every lane; lane i keeps the fired flag of
// chunk base + i, so each group's flags leave in one coalesced store.  Chunks of the tile past the recording's end get 0.
__global__ __launch_bounds__(64) void scan_trigger_kernel(const int32_t *__restrict__ index, const double *__restrict__ score, int n_chunks,
                                                          const int32_t *__restrict__ rec_chunks, long k0, int background, double sensitivity,
                                                          int level, int refractory, long out_stride, int32_t *__restrict__ state,
                                                          int32_t *__restrict__ fired)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const long live = clamp_chunks((long)rec_chunks[r] - k0, n_chunks);         // chunks of this tile the recording still has
    int32_t st[2] = {state[2 * (long)r], state[2 * (long)r + 1]};
    int32_t *row_fired = fired + r * out_stride;
    int mine = 0;
    walk_chunks(index + r * out_stride, score + r * out_stride, live,
                [&](int k, int idx, double sc) {
                    const int f = trigger_one(idx, sc, background, sensitivity, level, refractory, st);
                    if ((k & 63) == lane) mine = f;
                },
                [&](long base) {
                    if (base + lane < n_chunks) row_fired[base + lane] = mine;
                    mine = 0;
                });
    for (long i = ((live + 63) & ~63L) + lane; i < n_chunks; i += 64) row_fired[i] = 0;
    if (lane == 0) { state[2 * (long)r] = st[0]; state[2 * (long)r + 1] = st[1]; }
}

// The labelled events of one recording against the chunks of a walk that only moves forward.  The events are sorted and their chunk
// ranges lo .. hi disjoint (kws_amd.stream.events_to_chunks), so one cursor serves: e, the first event that does not end before the
// chunk last asked about.  Without labels (ev_off == nullptr) there are no events; the kernels say what a fire is then.
struct EventMatcher {
    const int32_t *cls, *lo, *hi;
    int begin, end, e;
    bool labelled, found;                                                       // found: event e already detected

    __device__ __forceinline__ EventMatcher(const int32_t *ev_off, const int32_t *ev_class, const int32_t *ev_lo, const int32_t *ev_hi, int r)
        : cls(ev_class), lo(ev_lo), hi(ev_hi), labelled(ev_off != nullptr), found(false)
    {
        begin = e = labelled ? ev_off[r] : 0;
        end = labelled ? ev_off[r + 1] : 0;
    }
    __device__ __forceinline__ void advance(int k)
    {
        while (e < end && hi[e] < k) { e += 1; found = false; }
    }
    // after advance(k): chunk k lies in event e's range
    __device__ __forceinline__ bool inside(int k) const { return e < end && lo[e] <= k; }
    // A fire of class c at chunk k: the first one inside an event of its class is the hit, later ones are duplicates, and a fire
    // outside every range, or of the wrong class inside one, is a false alarm.  `event` is the event's position among the
    // recording's (-1 for a false alarm); the cursor stays on it.
    __device__ __forceinline__ int classify(int k, int c, int &event)
    {
        advance(k);
        event = -1;
        if (!inside(k) || cls[e] != c) return KWS_DET_FALSE_ALARM;
        event = e - begin;
        if (found) return KWS_DET_DUPLICATE;
        found = true;
        return KWS_DET_HIT;
    }
};

// Operating-point sweep.  block = one wave = (recording r, 64 operating points): lane l owns point p = 64 blockIdx.y + l and carries
// ITS detector state, event matcher and counters in registers, all fed by the one walk.  A lane with p >= P walks like the others
// (the loads and broadcasts need the whole wave) with a level no activation count exceeds, and stores nothing.  counts (R, P, 5) =
// {fires, hits, false alarms, duplicates, sum over hits of (fire chunk - event's first chunk)}; every cell has one writer.
__global__ __launch_bounds__(64) void sweep_kernel(const int32_t *__restrict__ index, const double *__restrict__ score, long stride,
                                                   const int32_t *__restrict__ rec_chunks, int background, int refractory,
                                                   const double *__restrict__ sensitivity, const int32_t *__restrict__ trigger_level, int P,
                                                   const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_class,
                                                   const int32_t *__restrict__ ev_lo, const int32_t *__restrict__ ev_hi,
                                                   int32_t *__restrict__ counts)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const int p = blockIdx.y * 64 + lane;
    const bool owner = p < P;
    const double sens = owner ? sensitivity[p] : 0.0;
    const int level = owner ? trigger_level[p] : 0x7fffffff;
    EventMatcher events(ev_off, ev_class, ev_lo, ev_hi, r);
    int32_t st[2] = {0, -1};
    int fires = 0, hits = 0, false_alarms = 0, duplicates = 0, latency = 0;
    walk_chunks(index + r * stride, score + r * stride, clamp_chunks(rec_chunks[r], stride), [&](int k, int idx, double sc) {
        if (!trigger_one(idx, sc, background, sens, level, refractory, st)) return;
        fires += 1;
        if (!events.labelled) return;
        int event;
        const int kind = events.classify(k, idx, event);
        if (kind == KWS_DET_HIT) {
            hits += 1;
            latency += k - ev_lo[events.e];                                     // the cursor is on the event that was hit
        } else if (kind == KWS_DET_DUPLICATE) {
            duplicates += 1;
        } else {
            false_alarms += 1;
        }
    }, [](long) {});
    if (!owner) return;
    int32_t *out = counts + ((long)r * P + p) * 5;
    out[0] = fires; out[1] = hits; out[2] = false_alarms; out[3] = duplicates; out[4] = latency;
}

// Activations of one operating point.  block = one wave = one recording: the walk with ONE state, so state, event matcher and write
// position are wave-uniform (scalar registers); lane 0 stores each record, and the whole wave fills the unused slots afterwards.
// det (R, max_det, 4) = {chunk, class, kind, event}; the first max_det activations are kept, all are counted.
// The walk is written out here, the one kernel that does not call walk_chunks: with everything in scalar registers the compiler
// turned the call's step into a per-chunk path with four more register copies, and the kernel measured 3 % slower
// (profiles/stream_walk_speed.txt).  A change to walk_chunks belongs here too.
__global__ __launch_bounds__(64) void collect_kernel(const int32_t *__restrict__ index, const double *__restrict__ score, long stride,
                                                     const int32_t *__restrict__ rec_chunks, int background, int refractory, double sensitivity,
                                                     int level, const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_class,
                                                     const int32_t *__restrict__ ev_lo, const int32_t *__restrict__ ev_hi, int max_det,
                                                     int32_t *__restrict__ n_det, int32_t *__restrict__ det, double *__restrict__ det_score)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    EventMatcher events(ev_off, ev_class, ev_lo, ev_hi, r);
    int32_t st[2] = {0, -1};
    int n = 0;
    int32_t *out = det + (long)r * max_det * 4;
    double *out_score = det_score + (long)r * max_det;
    const long T = clamp_chunks(rec_chunks[r], stride);
    for (long base = 0; base < T; base += 64) {                                 // walk_chunks, written out (see above)
        const long i = base + lane;
        int idx = -1;
        double sc = 0.0;
        if (i < T) { idx = index[r * stride + i]; sc = score[r * stride + i]; }
        const int m = (int)(T - base < 64 ? T - base : 64);
        for (int j = 0; j < m; ++j) {
            const int ij = lane_value(idx, j);
            const double sj = lane_value(sc, j);
            if (!trigger_one(ij, sj, background, sensitivity, level, refractory, st)) continue;
            const int k = (int)base + j;
            int kind = KWS_DET_UNLABELLED, event = -1;
            if (events.labelled) kind = events.classify(k, ij, event);
            if (n < max_det && lane == 0) {
                out[4 * n] = k; out[4 * n + 1] = ij; out[4 * n + 2] = kind; out[4 * n + 3] = event;
                out_score[n] = sj;
            }
            n += 1;
        }
    }
    if (lane == 0) n_det[r] = n;
    for (int s = (n < max_det ? n : max_det) + lane; s < max_det; s += 64) {
        out[4 * s] = -1; out[4 * s + 1] = -1; out[4 * s + 2] = KWS_DET_UNLABELLED; out[4 * s + 3] = -1;
        out_score[s] = 0.0;
    }
}

// One lane's candidate peak; `chunk` kNoPeak = none.  The order is score descending, then chunk ascending: total over the candidates
// of a recording (chunks are distinct), so the maximum does not depend on the order in which lanes are combined.
struct Peak {
    double score;
    int chunk;
};
constexpr int kNoPeak = 0x7fffffff;

__device__ __forceinline__ Peak better_of(const Peak &a, const Peak &b)
{
    return (b.score > a.score || (b.score == a.score && b.chunk < a.chunk)) ? b : a;
}

// the value of the lane a DPP control names, all 64 lanes active (every control used below names a lane of the same row)
template <int kCtrl>
__device__ __forceinline__ Peak dpp_peak(const Peak &p)
{
    const int hi = __double2hiint(p.score), lo = __double2loint(p.score);
    Peak q;
    q.score = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xf, 0xf, false),
                               __builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xf, 0xf, false));
    q.chunk = __builtin_amdgcn_update_dpp(p.chunk, p.chunk, kCtrl, 0xf, 0xf, false);
    return q;
}

// Maximum of the wave's 64 candidates, the same in every lane.  Inside a row of 16 lanes four DPP exchanges (lane ^ 1, lane ^ 2, the
// mirror of each half row, the mirror of the row) leave the row's maximum in all of its lanes; the four rows are then read with
// v_readlane and combined in scalar registers.  No LDS, no atomics.
__device__ __forceinline__ Peak wave_best(Peak p)
{
    p = better_of(p, dpp_peak<0xB1>(p));                                        // quad_perm:[1,0,3,2]
    p = better_of(p, dpp_peak<0x4E>(p));                                        // quad_perm:[2,3,0,1]
    p = better_of(p, dpp_peak<0x141>(p));                                       // row_half_mirror
    p = better_of(p, dpp_peak<0x140>(p));                                       // row_mirror
    Peak w;
    w.score = lane_value(p.score, 0);
    w.chunk = lane_value(p.chunk, 0);
#pragma unroll
    for (int row = 1; row < 4; ++row) {
        Peak q;
        q.score = lane_value(p.score, 16 * row);
        q.chunk = lane_value(p.chunk, 16 * row);
        w = better_of(w, q);
    }
    return w;
}

// Near misses.  block = one wave = one recording, K <= 64 greedy picks.  For every pick the lanes stride over the recording's chunks
// (lane l sees l, l + 64, ... in ascending order, so a strict `>` keeps the lowest chunk among its equal scores) and each keeps its
// best candidate that is min_gap away from every earlier pick; wave_best names the winner.  Pick j lives in lane j's `mine`
// and is handed to the gap test by v_readlane.  The (index, score) rows are re-read per pick: they are a few KiB and stay in cache.
__global__ __launch_bounds__(64) void peaks_kernel(const int32_t *__restrict__ index, const double *__restrict__ score, long stride,
                                                   const int32_t *__restrict__ rec_chunks, int background, double min_score, int min_gap,
                                                   const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_lo,
                                                   const int32_t *__restrict__ ev_hi, int K, int32_t *__restrict__ n_peaks,
                                                   int32_t *__restrict__ peaks, double *__restrict__ peak_score)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const long T = clamp_chunks(rec_chunks[r], stride);
    const EventMatcher events(ev_off, nullptr, ev_lo, ev_hi, r);
    const int32_t *row_index = index + r * stride;
    const double *row_score = score + r * stride;
    int32_t *out = peaks + (long)r * K * 2;
    double *out_score = peak_score + (long)r * K;
    int mine = -1;                                                              // lane j: the chunk of pick j
    int n = 0;
    for (; n < K; ++n) {
        Peak best;
        best.score = -INFINITY;
        best.chunk = kNoPeak;
        EventMatcher mine_events = events;                                      // this lane's cursor, from the start: its chunks ascend
        for (long base = 0; base < T; base += 64) {
            const long k = base + lane;
            double sc = 0.0;
            bool cand = false;
            if (k < T) {
                sc = row_score[k];
                cand = row_index[k] != background && sc > min_score && sc > best.score;
                if (cand) {                                                     // inside an event's window, whatever its class: not a negative
                    mine_events.advance((int)k);
                    if (mine_events.inside((int)k)) cand = false;
                }
            }
            if (__builtin_amdgcn_ballot_w64(cand) == 0) continue;
            for (int j = 0; j < n; ++j) {                                       // wave-uniform trip count
                const long d = k - (long)lane_value(mine, j);
                if ((d < 0 ? -d : d) < (long)min_gap) cand = false;
            }
            if (cand) { best.score = sc; best.chunk = (int)k; }
        }
        const Peak w = wave_best(best);
        if (w.chunk == kNoPeak) break;
        if (lane == n) mine = w.chunk;
        if (lane == 0) {
            out[2 * n] = w.chunk; out[2 * n + 1] = row_index[w.chunk];
            out_score[n] = w.score;
        }
    }
    if (lane == 0) n_peaks[r] = n;
    for (int s = n + lane; s < K; s += 64) {
        out[2 * s] = -1; out[2 * s + 1] = -1;
        out_score[s] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Ragged streaming (kws_amd.stream.StreamServer): S slots, of which the A named in a push's table advance, each by a chunk of
// its own length.  An entry of the table is KWS_RAGGED_FIELDS int32: slot, the carry length the host mirrors, the chunk's
// length, the rows the push gives the slot, and a flag that restarts the slot first.  Every kernel clamps what it reads from
// the table to its buffers, so a wrong table gives wrong numbers and never an access outside them.
// ---------------------------------------------------------------------------------------------------------------------
using short8 = __attribute__((ext_vector_type(8))) short;
constexpr int kRaggedStep = 256 * 8;                                            // samples a block moves per pass, 16 bytes per thread

// block = one entry.  Carry and chunk are staged once in LDS (carry + chunk <= cap samples); after the barrier the LDS copy is the
// only source, so the compact row act[a] and the slot's post-push carry are written from it in the same kernel: the carry's shift
// cannot overlap its own reads and needs no second pass.  Rows of win / act (and of chunks when chunks_wide) start on 16 bytes
// and are a multiple of 8 samples long: that side moves 16 bytes per thread, the side whose offset is arbitrary (the chunk's
// place behind the carry, the carry's place inside the row) moves sample by sample through LDS.
__global__ __launch_bounds__(256) void ragged_append_kernel(short *__restrict__ win, long win_stride, int S, int cap,
                                                             const short *__restrict__ chunks, long chunk_stride, int chunks_wide,
                                                             const int32_t *__restrict__ table, int chunk_size, int W, int H,
                                                             short *__restrict__ act, long act_stride, int32_t *__restrict__ act_len)
{
    extern __shared__ __attribute__((aligned(16))) short ragged_lds[];         // cap samples, rounded up to 8
    const int a = blockIdx.x, t = threadIdx.x;
    const int32_t *e = table + (long)a * KWS_RAGGED_FIELDS;
    const int slot = e[KWS_RAGGED_SLOT];
    if (slot < 0 || slot >= S) {                                                // block-uniform
        if (t == 0) act_len[a] = 0;
        return;
    }
    int carry = e[KWS_RAGGED_RESET] ? 0 : e[KWS_RAGGED_CARRY];
    carry = carry < 0 ? 0 : (carry < cap ? carry : cap);
    int room = cap - carry;
    room = room < chunk_size ? room : chunk_size;
    room = (long)room < chunk_stride ? room : (int)chunk_stride;
    int len = e[KWS_RAGGED_LEN];
    len = len < 0 ? 0 : (len < room ? len : room);
    const int L = carry + len;
    short *w = win + (long)slot * win_stride;
    const short *c = chunks + (long)a * chunk_stride;
    for (int i = t * 8; i < carry; i += kRaggedStep) {
        const short8 v = *reinterpret_cast<const short8 *>(w + i);
        if (i + 8 <= carry) {
            *reinterpret_cast<short8 *>(ragged_lds + i) = v;
        } else {                                                                // the chunk's first samples share this vector
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i + j < carry) ragged_lds[i + j] = v[j];
        }
    }
    if (chunks_wide) {
        for (int i = t * 8; i < len; i += kRaggedStep) {
            const short8 v = *reinterpret_cast<const short8 *>(c + i);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i + j < len) ragged_lds[carry + i + j] = v[j];
        }
    } else {
        for (int i = t; i < len; i += 256) ragged_lds[carry + i] = c[i];
    }
    __syncthreads();
    short *o = act + (long)a * act_stride;
    for (int i = t * 8; i < L; i += kRaggedStep) {
        short8 v = *reinterpret_cast<const short8 *>(ragged_lds + i);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i + j >= L) v[j] = 0;
        *reinterpret_cast<short8 *>(o + i) = v;
    }
    if (t == 0) act_len[a] = L;
    const int n_new = L < W ? 0 : (L - W) / H + 1;                              // listen.py:103-105
    const long used = (long)n_new * H;
    const int keep = used < L ? (int)(L - used) : 0;                            // hop > window: the rows may consume more than is held
    for (int i = t * 8; i < keep; i += kRaggedStep) {
        short8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i + j < keep ? ragged_lds[used + i + j] : (short)0;
        *reinterpret_cast<short8 *>(w + i) = v;
    }
}

// block = one entry: push_rows_kernel's pass for the entry's slot with the entry's own row count, the updated window written a second
// time, compact, to feat[a] for the forward pass.
__global__ __launch_bounds__(256) void ragged_push_rows_kernel(float *__restrict__ mfccs, int S, int F, int D, const float *__restrict__ rows,
                                                                int max_frames, const int32_t *__restrict__ table, float *__restrict__ feat)
{
    const int a = blockIdx.x;
    const int32_t *e = table + (long)a * KWS_RAGGED_FIELDS;
    const int slot = e[KWS_RAGGED_SLOT];
    if (slot < 0 || slot >= S) return;
    int n_new = e[KWS_RAGGED_NEW];
    n_new = n_new < 0 ? 0 : (n_new < max_frames ? n_new : max_frames);
    const int n_keep = n_new < F ? n_new : F;
    const bool reset = e[KWS_RAGGED_RESET] != 0;
    const bool store = reset || n_keep > 0;                                     // no new row: the window is only copied
    const float *r = rows + ((long)a * max_frames + (n_new - n_keep)) * D;      // the last n_keep new rows
    slide_window<true>(mfccs + (long)slot * F * D, r, F * D, n_keep * D, reset, store, feat + (long)a * F * D);
}

// one thread per entry: postprocess_kernel with the slot's own operating point and state; results go to the entry's place in the
// compact arrays and to the slot's place in the per-slot ones
__global__ __launch_bounds__(256) void ragged_postprocess_kernel(const float *__restrict__ probs, int A, int C, const int32_t *__restrict__ table,
                                                                  int S, int background, DecDev d, const double *__restrict__ sensitivity,
                                                                  const int32_t *__restrict__ level, int refractory, int32_t *__restrict__ state,
                                                                  int32_t *__restrict__ slot_index, double *__restrict__ slot_score,
                                                                  int32_t *__restrict__ slot_fired, int32_t *__restrict__ index,
                                                                  double *__restrict__ score, int32_t *__restrict__ fired)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const int32_t *e = table + (long)a * KWS_RAGGED_FIELDS;
    const int slot = e[KWS_RAGGED_SLOT];
    if (slot < 0 || slot >= S) { index[a] = -1; score[a] = 0.0; fired[a] = 0; return; }
    int32_t st[2] = {0, -1};
    if (!e[KWS_RAGGED_RESET]) { st[0] = state[2 * (long)slot]; st[1] = state[2 * (long)slot + 1]; }
    double sc;
    const int arg = argmax_decode(probs + (long)a * C, C, background, d, sc);
    const int f = trigger_one(arg, sc, background, sensitivity[slot], level[slot], refractory, st);
    state[2 * (long)slot] = st[0];
    state[2 * (long)slot + 1] = st[1];
    index[a] = arg; score[a] = sc; fired[a] = f;
    slot_index[slot] = arg; slot_score[slot] = sc; slot_fired[slot] = f;
}

static DecDev dec_dev(const kws_decoder *d)
{
    DecDev v;
    if (!d) {
        v.cd = nullptr; v.n = 0; v.min_out = 0; v.out_range = 0; v.center = 0.5; v.enabled = 0;
    } else {
        v.cd = d->d_cd; v.n = (long)d->n; v.min_out = d->min_out; v.out_range = d->out_range; v.center = d->center; v.enabled = 1;
    }
    return v;
}

// Python floor division of -(8 * 2048) by chunk_size (listen.py:549)
static int refractory_of(int chunk_size)
{
    const int a = -(8 * 2048);
    int q = a / chunk_size;
    if ((a % chunk_size != 0) && ((a < 0) != (chunk_size < 0))) --q;
    return q;
}

// Argument checks that several entry points share: KWS_OK, or the failure as fail() recorded it.
static int check_ragged_push(int A, int S)
{
    return A < 0 || S < 0 || A > S ? fail(KWS_ERR_INVALID, "bad ragged push: A=%d entries for S=%d slots", A, S) : KWS_OK;
}

static int check_chunk_numbers(int64_t stride)
{
    return stride >= 0x7fffffffLL ? fail(KWS_ERR_UNSUPPORTED, "rows of %lld chunks: a chunk number must fit 31 bits", (long long)stride) : KWS_OK;
}

// `rest`: the event arrays the kernel reads besides ev_off are all there; `names` says which they are
static int check_events(const int32_t *ev_off, bool rest, const char *names)
{
    return ev_off && !rest ? fail(KWS_ERR_INVALID, "null argument: ev_off without %s", names) : KWS_OK;
}

}  // namespace kws

using namespace kws;

extern "C" {

int kws_decoder_create(const double *mu_stds, int n, double center, int resolution, double min_z, double max_z, kws_decoder **out)
{
    if (!mu_stds || !out || n < 1) return fail(KWS_ERR_INVALID, "threshold_config needs at least one (mu, std) pair");
    if (resolution < 1) return fail(KWS_ERR_INVALID, "resolution must be positive, got %d", resolution);
    // listen.py:468-470: int() truncates toward zero
    double lo = mu_stds[0] + min_z * mu_stds[1], hi = mu_stds[0] + max_z * mu_stds[1];
    for (int i = 1; i < n; ++i) {
        lo = std::min(lo, mu_stds[2 * i] + min_z * mu_stds[2 * i + 1]);
        hi = std::max(hi, mu_stds[2 * i] + max_z * mu_stds[2 * i + 1]);
    }
    if (!(std::fabs(lo) < 1e6) || !(std::fabs(hi) < 1e6)) return fail(KWS_ERR_INVALID, "threshold_config out of range");
    auto *d = new kws_decoder();
    d->min_out = (int32_t)lo;
    const int32_t max_out = (int32_t)hi;
    d->out_range = max_out - d->min_out;
    d->center = center;
    d->d_cd = nullptr;
    const int64_t npts = (int64_t)resolution * d->out_range;
    if (npts < 0 || npts > (int64_t)1 << 26) { delete d; return fail(KWS_ERR_INVALID, "threshold table of %lld points", (long long)npts); }
    if (npts == 0) {
        d->cd.assign(1, 0.0);          // np.cumsum of the scalar 0.0 (listen.py:519-522 with an empty linspace)
    } else {
        // _calc_pd: np.linspace(min_out, max_out, npts) -> i * step + start, last point exactly max_out
        std::vector<double> dens((size_t)npts, 0.0);
        const double start = (double)d->min_out, stop = (double)max_out;
        const double step = npts > 1 ? (stop - start) / (double)(npts - 1) : 0.0;
        for (int c = 0; c < n; ++c) {
            const double mu = mu_stds[2 * c], sd = mu_stds[2 * c + 1];
            if (sd == 0.0) continue;                                       // pdf() returns 0, listen.py:491-492
            const double norm = 1.0 / (sd * std::sqrt(2 * M_PI)), den = 2 * (sd * sd);
            for (int64_t i = 0; i < npts; ++i) {
                const double x = (npts > 1 && i == npts - 1) ? stop : (double)i * step + start;
                const double a = x - mu;
                dens[(size_t)i] += norm * std::exp(-(a * a) / den);
            }
        }
        d->cd.resize((size_t)npts);
        const double div = (double)((int64_t)resolution * n);
        double run = 0.0;
        for (int64_t i = 0; i < npts; ++i) { run += dens[(size_t)i] / div; d->cd[(size_t)i] = run; }
    }
    d->n = (int64_t)d->cd.size();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        delete d;
        return fail(KWS_ERR_HIP, "no HIP device: the threshold decoder has no CPU fallback");
    }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d->d_cd), sizeof(double) * d->cd.size());
    if (e == hipSuccess) e = hipMemcpy(d->d_cd, d->cd.data(), sizeof(double) * d->cd.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d->d_cd) (void)hipFree(d->d_cd);
        delete d;
        return fail(KWS_ERR_HIP, "threshold table upload failed: %s", hipGetErrorString(e));
    }
    *out = d;
    return KWS_OK;
}

void kws_decoder_destroy(kws_decoder *d)
{
    if (!d) return;
    if (d->d_cd) (void)hipFree(d->d_cd);
    delete d;
}

int kws_decoder_info(const kws_decoder *d, int32_t *min_out, int32_t *out_range, int64_t *table_len)
{
    if (!d) return fail(KWS_ERR_INVALID, "null decoder");
    if (min_out) *min_out = d->min_out;
    if (out_range) *out_range = d->out_range;
    if (table_len) *table_len = d->n;
    return KWS_OK;
}

int kws_decoder_table(const kws_decoder *d, double *host_cd, size_t count)
{
    if (!d || !host_cd) return fail(KWS_ERR_INVALID, "null argument");
    if (count != d->cd.size()) return fail(KWS_ERR_INVALID, "table has %zu entries, caller asked for %zu", d->cd.size(), count);
    std::memcpy(host_cd, d->cd.data(), count * sizeof(double));
    return KWS_OK;
}

int kws_decoder_decode(const kws_decoder *d, const void *raw, int raw_dtype, double *decoded, int64_t n, void *stream)
{
    if (!d || (!raw && n > 0) || (!decoded && n > 0)) return fail(KWS_ERR_INVALID, "null argument");
    if (n < 0) return fail(KWS_ERR_INVALID, "negative count");
    if (n == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (raw_dtype == KWS_RAW_F64)
        KWS_LAUNCH("decode_kernel_f64", decode_kernel<double>, grid, block, 0, s, static_cast<const double *>(raw), decoded, (long)n, dec_dev(d));
    else if (raw_dtype == KWS_RAW_F32)
        KWS_LAUNCH("decode_kernel_f32", decode_kernel<float>, grid, block, 0, s, static_cast<const float *>(raw), decoded, (long)n, dec_dev(d));
    else
        return fail(KWS_ERR_INVALID, "unknown raw dtype %d", raw_dtype);
    KWS_LAUNCH_CHECK("decode_kernel");
    return KWS_OK;
}

int kws_decoder_encode(const kws_decoder *d, double threshold, double *raw_out)
{
    if (!d || !raw_out) return fail(KWS_ERR_INVALID, "null argument");
    // listen.py:510-517
    const double t = 0.5 * threshold / d->center;
    const double cp = t < 0.5 ? t * d->center * 2 : (t - 0.5) * 2 * (1 - d->center) + d->center;
    const double ratio = (double)(std::lower_bound(d->cd.begin(), d->cd.end(), cp) - d->cd.begin()) / (double)d->cd.size();
    *raw_out = 1.0 / (1.0 + std::exp(-((double)d->min_out + (double)d->out_range * ratio)));
    return KWS_OK;
}

int kws_stream_push_rows(float *feat, const float *rows, int S, int F, int D, int n_rows, void *stream)
{
    if (S < 0 || F < 1 || D < 1 || n_rows < 0) return fail(KWS_ERR_INVALID, "bad stream geometry S=%d F=%d D=%d n_rows=%d", S, F, D, n_rows);
    if (S == 0 || n_rows == 0) return KWS_OK;
    if (!feat || !rows) return fail(KWS_ERR_INVALID, "null argument");
    KWS_LAUNCH("push_rows_kernel", push_rows_kernel, dim3((unsigned)S), dim3(256), 0, static_cast<hipStream_t>(stream), feat, rows, F, D,
               n_rows, std::min(n_rows, F));
    KWS_LAUNCH_CHECK("push_rows_kernel");
    return KWS_OK;
}

int kws_trigger_update(const int32_t *index, const double *score, int S, int background_index, double sensitivity, int trigger_level,
                       int chunk_size, int32_t *state, int32_t *fired, void *stream)
{
    if (S < 0 || chunk_size == 0) return fail(KWS_ERR_INVALID, "bad S=%d or chunk_size=%d", S, chunk_size);
    if (S == 0) return KWS_OK;
    if (!index || !score || !state || !fired) return fail(KWS_ERR_INVALID, "null argument");
    KWS_LAUNCH("trigger_kernel", trigger_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), index,
               score, S, background_index, sensitivity, trigger_level, refractory_of(chunk_size), state, fired);
    KWS_LAUNCH_CHECK("trigger_kernel");
    return KWS_OK;
}

int kws_stream_postprocess(const kws_decoder *dec, const float *probs, int S, int C, int background_index, double sensitivity,
                           int trigger_level, int chunk_size, int32_t *state, int32_t *index, double *score, int32_t *fired,
                           void *stream)
{
    if (S < 0 || C < 1 || chunk_size == 0) return fail(KWS_ERR_INVALID, "bad S=%d C=%d chunk_size=%d", S, C, chunk_size);
    if (S == 0) return KWS_OK;
    if (!probs || !state || !index || !score || !fired) return fail(KWS_ERR_INVALID, "null argument");
    KWS_LAUNCH("postprocess_kernel", postprocess_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
               probs, S, C, background_index, dec_dev(dec), sensitivity, trigger_level, refractory_of(chunk_size), state, index, score,
               fired);
    KWS_LAUNCH_CHECK("postprocess_kernel");
    return KWS_OK;
}

static bool on_16_bytes(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int kws_stream_ragged_append(int16_t *win, int64_t win_stride, int S, int cap, const int16_t *chunks, int64_t chunk_stride,
                             const int32_t *table, int A, int chunk_size, int window_samples, int hop_samples, int16_t *act,
                             int64_t act_stride, int32_t *act_len, void *stream)
{
    if (int rc = check_ragged_push(A, S)) return rc;
    if (chunk_size < 1 || window_samples < 1 || hop_samples < 1)
        return fail(KWS_ERR_INVALID, "bad chunk_size=%d window=%d hop=%d", chunk_size, window_samples, hop_samples);
    if ((int64_t)cap < (int64_t)window_samples + chunk_size)
        return fail(KWS_ERR_INVALID, "cap=%d is less than window + chunk_size = %d + %d: a slot's carry and one chunk would not fit", cap,
                    window_samples, chunk_size);
    if (cap > 32768) return fail(KWS_ERR_UNSUPPORTED, "cap=%d samples: carry and chunk are staged in 64 KiB of LDS (at most 32768)", cap);
    if (win_stride < cap || act_stride < cap || (win_stride & 7) || (act_stride & 7) || chunk_stride < 1)
        return fail(KWS_ERR_INVALID, "bad strides win=%lld act=%lld chunks=%lld: win / act rows hold cap=%d samples and are a multiple of 8 long",
                    (long long)win_stride, (long long)act_stride, (long long)chunk_stride, cap);
    if (A == 0) return KWS_OK;
    if (!win || !chunks || !table || !act || !act_len) return fail(KWS_ERR_INVALID, "null argument");
    if (!on_16_bytes(win) || !on_16_bytes(act)) return fail(KWS_ERR_INVALID, "win and act must start on 16 bytes");
    const int wide = on_16_bytes(chunks) && (chunk_stride & 7) == 0;
    const size_t smem = sizeof(int16_t) * (size_t)((cap + 7) & ~7);
    KWS_LAUNCH("ragged_append_kernel", ragged_append_kernel, dim3((unsigned)A), dim3(256), smem, static_cast<hipStream_t>(stream),
               reinterpret_cast<short *>(win), (long)win_stride, S, cap, reinterpret_cast<const short *>(chunks), (long)chunk_stride, wide, table,
               chunk_size, window_samples, hop_samples, reinterpret_cast<short *>(act), (long)act_stride, act_len);
    KWS_LAUNCH_CHECK("ragged_append_kernel");
    return KWS_OK;
}

int kws_stream_ragged_push_rows(float *mfccs, int S, int F, int D, const float *rows, int max_frames, const int32_t *table, int A,
                                float *feat, void *stream)
{
    if (int rc = check_ragged_push(A, S)) return rc;
    if (F < 1 || D < 1 || max_frames < 0) return fail(KWS_ERR_INVALID, "bad stream geometry F=%d D=%d max_frames=%d", F, D, max_frames);
    if (A == 0) return KWS_OK;
    if (!mfccs || !table || !feat || (!rows && max_frames > 0)) return fail(KWS_ERR_INVALID, "null argument");
    KWS_LAUNCH("ragged_push_rows_kernel", ragged_push_rows_kernel, dim3((unsigned)A), dim3(256), 0, static_cast<hipStream_t>(stream), mfccs, S, F,
               D, rows, max_frames, table, feat);
    KWS_LAUNCH_CHECK("ragged_push_rows_kernel");
    return KWS_OK;
}

int kws_stream_ragged_postprocess(const kws_decoder *dec, const float *probs, int A, int C, const int32_t *table, int S, int background_index,
                                  const double *sensitivity, const int32_t *trigger_level, int chunk_size, int32_t *state,
                                  int32_t *slot_index, double *slot_score, int32_t *slot_fired, int32_t *index, double *score, int32_t *fired,
                                  void *stream)
{
    if (int rc = check_ragged_push(A, S)) return rc;
    if (C < 1 || chunk_size < 1) return fail(KWS_ERR_INVALID, "bad C=%d chunk_size=%d", C, chunk_size);
    if (A == 0) return KWS_OK;
    if (!probs || !table || !sensitivity || !trigger_level || !state || !slot_index || !slot_score || !slot_fired || !index || !score || !fired)
        return fail(KWS_ERR_INVALID, "null argument");
    KWS_LAUNCH("ragged_postprocess_kernel", ragged_postprocess_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0,
               static_cast<hipStream_t>(stream), probs, A, C, table, S, background_index, dec_dev(dec), sensitivity, trigger_level,
               refractory_of(chunk_size), state, slot_index, slot_score, slot_fired, index, score, fired);
    KWS_LAUNCH_CHECK("ragged_postprocess_kernel");
    return KWS_OK;
}

int kws_stream_gather_windows(const float *rows, int R, int max_frames, const int32_t *lengths, int chunk_size, int window_samples,
                              int hop_samples, int F, int D, int64_t k0, int n_chunks, float *feat, void *stream)
{
    if (R < 0 || n_chunks < 0 || max_frames < 0 || k0 < 0) return fail(KWS_ERR_INVALID, "bad scan geometry R=%d n_chunks=%d max_frames=%d", R, n_chunks, max_frames);
    if (chunk_size < 1 || window_samples < 1 || hop_samples < 1 || F < 1 || D < 1)
        return fail(KWS_ERR_INVALID, "bad chunk_size=%d window=%d hop=%d F=%d D=%d", chunk_size, window_samples, hop_samples, F, D);
    if (hop_samples > window_samples)
        return fail(KWS_ERR_INVALID, "hop=%d > window=%d: the chunk loop's frames do not start on multiples of the hop, the scan's closed form "
                                     "does not hold", hop_samples, window_samples);
    if (R == 0 || n_chunks == 0) return KWS_OK;
    if (!lengths || !feat || (!rows && max_frames > 0)) return fail(KWS_ERR_INVALID, "null argument");
    const long n_windows = (long)R * n_chunks;
    KWS_LAUNCH("gather_windows_kernel", gather_windows_kernel, dim3((unsigned)std::min<long>(n_windows, 1L << 20)), dim3(256), 0,
               static_cast<hipStream_t>(stream), rows, max_frames, lengths, chunk_size, window_samples, hop_samples, F, D, (long)k0, n_chunks,
               n_windows, feat);
    KWS_LAUNCH_CHECK("gather_windows_kernel");
    return KWS_OK;
}

int kws_stream_scan_postprocess(const kws_decoder *dec, const float *probs, int R, int n_chunks, int C, const int32_t *rec_chunks, int64_t k0,
                                int background_index, double sensitivity, int trigger_level, int chunk_size, int32_t *state, int32_t *index,
                                double *score, int32_t *fired, int64_t out_stride, void *stream)
{
    if (R < 0 || n_chunks < 0 || C < 1 || chunk_size == 0 || k0 < 0) return fail(KWS_ERR_INVALID, "bad R=%d n_chunks=%d C=%d chunk_size=%d", R, n_chunks, C, chunk_size);
    if (out_stride < n_chunks) return fail(KWS_ERR_INVALID, "out_stride=%lld is shorter than the tile's %d chunks", (long long)out_stride, n_chunks);
    if (R == 0 || n_chunks == 0) return KWS_OK;
    if (!probs || !rec_chunks || !state || !index || !score || !fired) return fail(KWS_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long n_windows = (long)R * n_chunks;
    if ((n_windows + 255) / 256 > 0x7fffffffL) return fail(KWS_ERR_UNSUPPORTED, "%ld windows in one tile", n_windows);
    KWS_LAUNCH("scan_decode_kernel", scan_decode_kernel, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, s, probs, n_chunks, C, rec_chunks,
               (long)k0, background_index, dec_dev(dec), n_windows, (long)out_stride, index, score);
    KWS_LAUNCH_CHECK("scan_decode_kernel");
    KWS_LAUNCH("scan_trigger_kernel", scan_trigger_kernel, dim3((unsigned)R), dim3(64), 0, s, index, score, n_chunks, rec_chunks, (long)k0,
               background_index, sensitivity, trigger_level, refractory_of(chunk_size), (long)out_stride, state, fired);
    KWS_LAUNCH_CHECK("scan_trigger_kernel");
    return KWS_OK;
}

int kws_stream_sweep(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks, int background_index,
                     int chunk_size, const double *sensitivity, const int32_t *trigger_level, int P, const int32_t *ev_off,
                     const int32_t *ev_class, const int32_t *ev_lo, const int32_t *ev_hi, int32_t *counts, void *stream)
{
    if (R < 0 || P < 0 || stride < 0 || chunk_size < 1) return fail(KWS_ERR_INVALID, "bad R=%d P=%d stride=%lld chunk_size=%d", R, P, (long long)stride, chunk_size);
    if (R == 0 || P == 0) return KWS_OK;
    if (!rec_chunks || !sensitivity || !trigger_level || !counts || ((!index || !score) && stride > 0)) return fail(KWS_ERR_INVALID, "null argument");
    const long groups = ((long)P + 63) / 64;
    if (groups > 65535) return fail(KWS_ERR_UNSUPPORTED, "%d operating points in one sweep (at most %d)", P, 65535 * 64);
    KWS_LAUNCH("sweep_kernel", sweep_kernel, dim3((unsigned)R, (unsigned)groups), dim3(64), 0, static_cast<hipStream_t>(stream), index, score,
               (long)stride, rec_chunks, background_index, refractory_of(chunk_size), sensitivity, trigger_level, P, ev_off, ev_class, ev_lo, ev_hi,
               counts);
    KWS_LAUNCH_CHECK("sweep_kernel");
    return KWS_OK;
}

int kws_stream_collect(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks, int background_index,
                       int chunk_size, double sensitivity, int trigger_level, const int32_t *ev_off, const int32_t *ev_class,
                       const int32_t *ev_lo, const int32_t *ev_hi, int max_det, int32_t *n_det, int32_t *det, double *det_score, void *stream)
{
    if (R < 0 || stride < 0 || chunk_size < 1 || max_det < 0)
        return fail(KWS_ERR_INVALID, "bad R=%d stride=%lld chunk_size=%d max_det=%d", R, (long long)stride, chunk_size, max_det);
    if (int rc = check_chunk_numbers(stride)) return rc;
    if (R == 0) return KWS_OK;
    if (!rec_chunks || !n_det || ((!index || !score) && stride > 0) || ((!det || !det_score) && max_det > 0))
        return fail(KWS_ERR_INVALID, "null argument");
    if (int rc = check_events(ev_off, ev_class && ev_lo && ev_hi, "ev_class / ev_lo / ev_hi")) return rc;
    KWS_LAUNCH("collect_kernel", collect_kernel, dim3((unsigned)R), dim3(64), 0, static_cast<hipStream_t>(stream), index, score, (long)stride,
               rec_chunks, background_index, refractory_of(chunk_size), sensitivity, trigger_level, ev_off, ev_class, ev_lo, ev_hi, max_det,
               n_det, det, det_score);
    KWS_LAUNCH_CHECK("collect_kernel");
    return KWS_OK;
}

int kws_stream_peaks(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks, int background_index,
                     double min_score, int min_gap, const int32_t *ev_off, const int32_t *ev_lo, const int32_t *ev_hi, int K,
                     int32_t *n_peaks, int32_t *peaks, double *peak_score, void *stream)
{
    if (K < 1 || K > 64) return fail(KWS_ERR_INVALID, "K=%d peaks per recording is outside 1..64", K);
    if (min_gap < 1) return fail(KWS_ERR_INVALID, "min_gap=%d must be at least 1", min_gap);
    if (R < 0 || stride < 0) return fail(KWS_ERR_INVALID, "bad R=%d stride=%lld", R, (long long)stride);
    if (int rc = check_chunk_numbers(stride)) return rc;
    if (R == 0) return KWS_OK;
    if (!rec_chunks || !n_peaks || !peaks || !peak_score || ((!index || !score) && stride > 0)) return fail(KWS_ERR_INVALID, "null argument");
    if (int rc = check_events(ev_off, ev_lo && ev_hi, "ev_lo / ev_hi")) return rc;
    KWS_LAUNCH("peaks_kernel", peaks_kernel, dim3((unsigned)R), dim3(64), 0, static_cast<hipStream_t>(stream), index, score, (long)stride,
               rec_chunks, background_index, min_score, min_gap, ev_off, ev_lo, ev_hi, K, n_peaks, peaks, peak_score);
    KWS_LAUNCH_CHECK("peaks_kernel");
    return KWS_OK;
}

}  // extern "C"
