// csrc/kws_dtw.hip -- query-by-example keyword search: subsequence dynamic time warping of templates against recordings
// (include/kws.h): kws_dtw_workspace_bytes, kws_dtw, kws_dtw_peaks.
//
// dtw_kernel: one wave per (recording, template, tile of frames) job.  Lane i owns template row i, with q_i in registers for the
// whole job, and the wave walks the frames one column per step: ALL lanes are at column j at step j.  The recurrence has no
// predecessor in its own column -- (i-1, j-1), (i-1, j-2) and (i-2, j-1) all lie in earlier columns -- so the anti-diagonal skew a
// DTW with a vertical step needs buys nothing here: without it there is no fill and drain of 2 (L - 1) steps per job, and the row
// x_j every lane multiplies with is ONE address for the wave, a broadcast read of LDS that no stride can make collide.  A lane
// keeps (C, S) of its last column; lane i - 1's and lane i - 2's come through DPP wave shifts (v_mov_b32 wave_shr:1, once and
// twice), and lane i - 1's pair of the column before is the shift the lane already made one step earlier.  Nothing of the DP
// touches memory.  The rows are staged in LDS in chunks of 64 columns with 128-bit loads, the next chunk's loads in flight under
// the current chunk's steps; the local cost is a chain of D FMAs per lane and step in ascending column order, which depends on
// the two rows only.  Row L - 1's pair is picked with v_readlane into the lane that owns the column's output slot, and a chunk's
// 64 costs and starts leave as two coalesced vector stores.
// Tiles: a job starts its DP at the tile's first frame minus a halo of 2 (L - 1) frames (rounded down to a chunk).  Every path to
// (L - 1, j) lies in the columns >= j - 2 (L - 1), and every cell on such a path has all of ITS paths inside the halo too, so a
// tile computes the same minimum over the same sums, added in the same order, as an unsplit recording: the same bits for every
// tile size.  Jobs are planned from R, Q and max_frames alone; the lengths are read on the device.  No atomics.
// dtw_peaks_kernel: one wave per (recording, keyword), greedy selection in a total order (value, then frame, then template).
#include <climits>
#include <cmath>

#include "kws_common.h"

namespace kws {

namespace {

constexpr int kDtwChunk = 64;              // columns staged at a time: one output slot per lane
constexpr int kDtwMinTile = 32, kDtwMaxTile = 1 << 20;
constexpr int kDtwMaxFrames = 1 << 30;      // column indices and their chunk arithmetic stay inside an int
constexpr int kDtwAutoMinTile = 256;       // the library's own cut: the halo (up to 126 + 63 frames) stays a fraction of a tile
constexpr int kDtwAutoJobs = 4096;         // ... and there are about this many waves where the frames allow it (256 CUs x 16)
constexpr int kDtwPeakMaxQ = 1024;         // templates of one kws_dtw_peaks call: the member list of a keyword lives in LDS

inline int64_t dtw_tile(int64_t R, int64_t Q, int64_t max_frames, int tile_frames)
{
    if (tile_frames) return tile_frames;
    const int64_t pairs = std::max<int64_t>(1, R * Q);
    const int64_t tiles = (kDtwAutoJobs + pairs - 1) / pairs;
    int64_t T = (max_frames + tiles - 1) / tiles;
    T = (T + kDtwChunk - 1) / kDtwChunk * kDtwChunk;
    return std::min<int64_t>(std::max<int64_t>(T, kDtwAutoMinTile), kDtwMaxTile);
}

// lane i takes lane i - 1's value, lane 0 takes `fill`
__device__ __forceinline__ float dtw_up1(float v, float fill)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ int dtw_up1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }

// NG: float4 groups of a staged row (the width D rounded up to 4, 12, 20, 32 or 64 columns; the zero columns change neither metric)
template <bool L2, int NG>
__global__ __launch_bounds__(64) void dtw_kernel(const float *__restrict__ templates, const int32_t *__restrict__ tmpl_len, int Q, int Lmax,
                                                 const float *__restrict__ rows, const int32_t *__restrict__ n_frames, int max_frames, int D,
                                                 int T, int ntiles, float *__restrict__ cost, int32_t *__restrict__ start)
{
#pragma clang fp contract(off)
    __shared__ float4 xs[2][kDtwChunk * NG];
    const int lane = threadIdx.x, d4 = D >> 2;
    const long job = blockIdx.x;
    const int q = (int)(job % Q), t = (int)((job / Q) % ntiles), r = (int)(job / Q / ntiles);
    int L = tmpl_len[q], n = n_frames[r];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    n = n < 0 ? 0 : (n > max_frames ? max_frames : n);
    const long t0 = (long)t * T;                                        // the job's outputs: frames [t0, t1)
    const int t1 = (int)(t0 + T < max_frames ? t0 + T : max_frames);
    const int stop = (L >= 1 && n > t0) ? (n < t1 ? n : t1) : 0;       // the DP runs over the columns [cb, stop)
    long cbl = stop ? t0 - 2 * (L - 1) : t0;
    const int cb = (int)(cbl < 0 ? 0 : cbl) & ~(kDtwChunk - 1);
    const int Lm1 = L >= 1 ? L - 1 : 0;

    float4 qv[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        qv[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < L && g < d4) qv[g] = *reinterpret_cast<const float4 *>(templates + ((long)q * Lmax + lane) * D + 4 * g);
    }
    float4 *xflat = &xs[0][0];
    for (int p = lane; p < 2 * kDtwChunk * NG; p += 64) xflat[p] = make_float4(0.f, 0.f, 0.f, 0.f);   // the padding columns stay zero

    // a chunk is kDtwChunk * d4 consecutive float4 of the recording: lane + 64 k is float4 (lane + 64 k) % d4 of row (lane + 64 k) / d4
    const float *rec = rows + (long)r * max_frames * D;
    float4 px[NG];
    auto fetch = [&](int c) {
        const long live = (long)(stop - c) * d4;                         // float4 of the chunk that belong to columns < stop
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int p = lane + 64 * k;
            px[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < d4 && p < live) px[k] = *reinterpret_cast<const float4 *>(rec + (long)c * D + 4 * (long)p);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int p = lane + 64 * k;
            if (k < d4) {
                const int row = p / d4, col = p - row * d4;
                xs[buf][row * NG + col] = px[k];
            }
        }
    };

    __syncthreads();
    if (cb < stop) { fetch(cb); stash(0); }
    __syncthreads();

    const float INF = INFINITY;
    float Cp = INF, ao = INF;             // this row's cost at the last column; row i - 1's at the column before that
    int Sp = -1, aoS = -1;
    int buf = 0;
    for (int c = cb; c < t1; c += kDtwChunk, buf ^= 1) {
        const bool more = c + kDtwChunk < stop;
        if (more) fetch(c + kDtwChunk);
        float outC = INF;
        int outS = -1;
        const int steps = stop - c < kDtwChunk ? stop - c : kDtwChunk;   // <= 0 past the recording's end
        const float4 *xr = xs[buf];
        for (int jj = 0; jj < steps; ++jj, xr += NG) {
            float acc = 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float4 x = xr[g];
                if (L2) {
                    const float e0 = qv[g].x - x.x, e1 = qv[g].y - x.y, e2 = qv[g].z - x.z, e3 = qv[g].w - x.w;
                    acc = fmaf(e0, e0, acc); acc = fmaf(e1, e1, acc); acc = fmaf(e2, e2, acc); acc = fmaf(e3, e3, acc);
                } else {
                    acc = fmaf(qv[g].x, x.x, acc); acc = fmaf(qv[g].y, x.y, acc); acc = fmaf(qv[g].z, x.z, acc); acc = fmaf(qv[g].w, x.w, acc);
                }
            }
            const float d = L2 ? acc : 1.f - acc;
            const float a = dtw_up1(Cp, INF), b = dtw_up1(a, INF);       // C(i-1, j-1), C(i-2, j-1)
            const int aS = dtw_up1(Sp, -1), bS = dtw_up1(aS, -1);
            const float c1 = a + d, c2 = ao + d, c3 = b + (d + d);
            float best = c1;
            int S = aS;
            if (c2 < best) { best = c2; S = aoS; }
            if (c3 < best) { best = c3; S = bS; }
            if (lane == 0) { best = d; S = c + jj; }
            if (!(best < INF)) { best = INF; S = -1; }
            ao = a; aoS = aS;
            Cp = best; Sp = S;
            const float oc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), Lm1));
            const int os = __builtin_amdgcn_readlane(S, Lm1);
            if (lane == jj) { outC = oc; outS = os; }
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
        const int j = c + lane;
        if (j >= t0 && j < t1) {
            const long o = ((long)r * Q + q) * max_frames + j;
            cost[o] = outC / (float)(L >= 1 ? L : 1);
            start[o] = outS;
        }
    }
}

// one wave per (recording, keyword): up to K rounds over the keyword's curve, the minimum over its templates
__global__ __launch_bounds__(64) void dtw_peaks_kernel(const float *__restrict__ cost, const int32_t *__restrict__ start, int Q, int max_frames,
                                                       const int32_t *__restrict__ group, int G, float threshold, int min_gap, int K,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ end, int32_t *__restrict__ hit_start,
                                                       float *__restrict__ hit_cost, int32_t *__restrict__ hit_template)
{
    __shared__ int members[kDtwPeakMaxQ];
    __shared__ int emitted[KWS_DTW_MAX_HITS];
    const int lane = threadIdx.x;
    const int r = blockIdx.x / G, g = blockIdx.x % G;
    int nm = 0;                                                          // the keyword's templates in ascending order
    for (int q0 = 0; q0 < Q; q0 += 64) {
        const int q = q0 + lane;
        const bool m = q < Q && group[q] == g;
        const unsigned long long bal = __ballot(m);
        if (m) members[nm + __popcll(bal & ((1ull << lane) - 1ull))] = q;
        nm += __popcll(bal);
    }
    __syncthreads();
    const float *cr = cost + (long)r * Q * max_frames;
    const long ob = ((long)r * G + g) * K;
    int ne = 0;
    for (int k = 0; k < K; ++k) {
        float bv = INFINITY;
        int bf = INT_MAX;
        for (int f = lane; f < max_frames; f += 64) {                    // ascending frames per lane: `<` keeps the lower frame
            float v = INFINITY;
            for (int m = 0; m < nm; ++m) {
                const float x = cr[(long)members[m] * max_frames + f];
                v = x < v ? x : v;
            }
            if (v < bv && v <= threshold && v > -INFINITY) {
                bool sup = false;
                for (int e = 0; e < ne; ++e) {
                    const long dl = (long)f - emitted[e];
                    sup |= (dl < 0 ? -dl : dl) < min_gap;
                }
                if (!sup) { bv = v; bf = f; }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int of = __shfl_xor(bf, o, 64);
            if (ov < bv || (ov == bv && of < bf)) { bv = ov; bf = of; }
        }
        if (bf == INT_MAX) break;                                        // the same value in every lane
        if (lane == 0) {
            int tq = -1;
            for (int m = 0; m < nm && tq < 0; ++m)
                if (cr[(long)members[m] * max_frames + bf] == bv) tq = members[m];     // the lowest template at the minimum
            end[ob + k] = bf;
            hit_start[ob + k] = tq >= 0 ? start[((long)r * Q + tq) * max_frames + bf] : -1;
            hit_cost[ob + k] = bv;
            hit_template[ob + k] = tq;
            emitted[ne] = bf;
        }
        ++ne;
        __syncthreads();
    }
    if (lane == 0) count[(long)r * G + g] = ne;
    for (int k = ne + lane; k < K; k += 64) {
        end[ob + k] = -1;
        hit_start[ob + k] = -1;
        hit_cost[ob + k] = INFINITY;
        hit_template[ob + k] = -1;
    }
}

int dtw_check_shape(const char *who, int64_t R, int64_t Q, int64_t max_frames, int D, int tile_frames)
{
    if (D < 4 || D > 64 || D % 4) return fail(KWS_ERR_INVALID, "%s: D = %d is not a multiple of 4 in 4 .. 64", who, D);
    if (R < 0 || Q < 0) return fail(KWS_ERR_INVALID, "%s: R = %lld recordings, Q = %lld templates", who, (long long)R, (long long)Q);
    if (max_frames < 1 || max_frames > kDtwMaxFrames) return fail(KWS_ERR_INVALID, "%s: max_frames = %lld outside 1 .. 2^30", who, (long long)max_frames);
    if (tile_frames != 0 && (tile_frames < kDtwMinTile || tile_frames > kDtwMaxTile))
        return fail(KWS_ERR_INVALID, "%s: tile_frames = %d is neither 0 nor in %d .. %d", who, tile_frames, kDtwMinTile, kDtwMaxTile);
    const int64_t T = dtw_tile(R, Q, max_frames, tile_frames), ntiles = (max_frames + T - 1) / T;
    if (R && Q && ntiles > (int64_t)INT_MAX / R / Q)
        return fail(KWS_ERR_UNSUPPORTED, "%s: %lld x %lld pairs of %lld frames are more than one launch takes", who, (long long)R, (long long)Q, (long long)max_frames);
    return KWS_OK;
}

template <bool L2>
int dtw_launch(int ng, int64_t jobs, hipStream_t s, const float *templates, const int32_t *tmpl_len, int Q, int Lmax, const float *rows,
               const int32_t *n_frames, int max_frames, int D, int T, int ntiles, float *cost, int32_t *start)
{
#define KWS_DTW_CASE(NG)                                                                                                                  \
    case NG:                                                                                                                              \
        KWS_LAUNCH("dtw_kernel", (dtw_kernel<L2, NG>), dim3((unsigned)jobs), dim3(64), 0, s, templates, tmpl_len, Q, Lmax, rows, n_frames, \
                   max_frames, D, T, ntiles, cost, start);                                                                                \
        break;
    switch (ng) {
        KWS_DTW_CASE(1)
        KWS_DTW_CASE(3)
        KWS_DTW_CASE(5)
        KWS_DTW_CASE(8)
        KWS_DTW_CASE(16)
    default: return fail(KWS_ERR_INVALID, "dtw: no kernel for %d column groups", ng);
    }
#undef KWS_DTW_CASE
    KWS_LAUNCH_CHECK("dtw_kernel");
    return KWS_OK;
}

}  // namespace

}  // namespace kws

using namespace kws;

extern "C" {

int64_t kws_dtw_workspace_bytes(int R, int Q, int max_frames, int D, int tile_frames)
{
    if (int rc = dtw_check_shape("dtw workspace", R, Q, max_frames, D, tile_frames)) return rc;
    return 0;             // the DP lives in registers and a tile recomputes its halo: nothing is handed from job to job
}

int kws_dtw(const float *templates, const int32_t *tmpl_len, int Q, int Lmax, const float *rows, const int32_t *n_frames, int R, int max_frames,
            int D, int metric, int tile_frames, float *cost, int32_t *start, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = dtw_check_shape("dtw", R, Q, max_frames, D, tile_frames)) return rc;
    if (Lmax < 1 || Lmax > KWS_DTW_MAX_ROWS) return fail(KWS_ERR_INVALID, "dtw: Lmax = %d template rows outside 1 .. %d", Lmax, KWS_DTW_MAX_ROWS);
    if (metric != KWS_DTW_DOT && metric != KWS_DTW_L2) return fail(KWS_ERR_INVALID, "dtw: metric = %d (KWS_DTW_DOT or KWS_DTW_L2)", metric);
    if (!templates || !tmpl_len || !rows || !n_frames || !cost || !start) return fail(KWS_ERR_INVALID, "dtw: null argument");
    if ((reinterpret_cast<uintptr_t>(templates) | reinterpret_cast<uintptr_t>(rows)) & 15)
        return fail(KWS_ERR_INVALID, "dtw: templates and rows must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(tmpl_len) | reinterpret_cast<uintptr_t>(n_frames) | reinterpret_cast<uintptr_t>(cost) | reinterpret_cast<uintptr_t>(start)) & 3)
        return fail(KWS_ERR_INVALID, "dtw: tmpl_len, n_frames, cost and start must be 4-byte aligned");
    const size_t need = (size_t)kws_dtw_workspace_bytes(R, Q, max_frames, D, tile_frames);
    if (need && (!ws || ws_bytes < need))
        return fail(KWS_ERR_WORKSPACE, "dtw: needs a workspace of %zu bytes (kws_dtw_workspace_bytes), got %zu", need, ws ? ws_bytes : (size_t)0);
    if (R == 0 || Q == 0) return KWS_OK;
    const int64_t T = std::min<int64_t>(dtw_tile(R, Q, max_frames, tile_frames), max_frames);
    const int64_t ntiles = (max_frames + T - 1) / T, jobs = (int64_t)R * Q * ntiles;
    const int d4 = D / 4, ng = d4 <= 1 ? 1 : d4 <= 3 ? 3 : d4 <= 5 ? 5 : d4 <= 8 ? 8 : 16;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return metric == KWS_DTW_L2
               ? dtw_launch<true>(ng, jobs, s, templates, tmpl_len, Q, Lmax, rows, n_frames, max_frames, D, (int)T, (int)ntiles, cost, start)
               : dtw_launch<false>(ng, jobs, s, templates, tmpl_len, Q, Lmax, rows, n_frames, max_frames, D, (int)T, (int)ntiles, cost, start);
}

int kws_dtw_peaks(const float *cost, const int32_t *start, int R, int Q, int max_frames, const int32_t *group, const int32_t *group_host, int G,
                  float threshold, int min_gap, int K, int32_t *count, int32_t *end, int32_t *hit_start, float *hit_cost, int32_t *hit_template,
                  void *stream)
{
    if (R < 0) return fail(KWS_ERR_INVALID, "dtw peaks: R = %d recordings", R);
    if (Q < 1 || Q > kDtwPeakMaxQ) return fail(KWS_ERR_INVALID, "dtw peaks: Q = %d templates outside 1 .. %d", Q, kDtwPeakMaxQ);
    if (max_frames < 1) return fail(KWS_ERR_INVALID, "dtw peaks: max_frames = %d", max_frames);
    if (G < 1 || G > Q) return fail(KWS_ERR_INVALID, "dtw peaks: G = %d keywords for %d templates", G, Q);
    if (K < 1 || K > KWS_DTW_MAX_HITS) return fail(KWS_ERR_INVALID, "dtw peaks: K = %d hits outside 1 .. %d", K, KWS_DTW_MAX_HITS);
    if (min_gap < 1) return fail(KWS_ERR_INVALID, "dtw peaks: min_gap = %d frames, at least 1", min_gap);
    if (threshold != threshold) return fail(KWS_ERR_INVALID, "dtw peaks: the threshold is NaN");
    if (!cost || !start || !group || !count || !end || !hit_start || !hit_cost || !hit_template) return fail(KWS_ERR_INVALID, "dtw peaks: null argument");
    if (group_host) {
        for (int q = 0; q < Q; ++q) {
            const int prev = q ? group_host[q - 1] : 0;
            if (group_host[q] < prev || group_host[q] > prev + (q ? 1 : 0))
                return fail(KWS_ERR_INVALID, "dtw peaks: group[%d] = %d after %d: the keywords must be non-decreasing from 0 without gaps", q, group_host[q], prev);
        }
        if (group_host[Q - 1] != G - 1) return fail(KWS_ERR_INVALID, "dtw peaks: the last template belongs to keyword %d of %d", group_host[Q - 1], G);
    }
    if ((int64_t)R * G > (int64_t)INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "dtw peaks: %d x %d curves are more than one launch takes", R, G);
    if (R == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    KWS_LAUNCH("dtw_peaks_kernel", dtw_peaks_kernel, dim3((unsigned)(R * G)), dim3(64), 0, s, cost, start, Q, max_frames, group, G, threshold, min_gap, K,
               count, end, hit_start, hit_cost, hit_template);
    KWS_LAUNCH_CHECK("dtw_peaks_kernel");
    return KWS_OK;
}

}  // extern "C"
