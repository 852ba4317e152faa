// csrc/kws_score.hip -- score statistics of an evaluated batch (include/kws.h: kws_score_hist): per-class target /
// non-target score histograms, the rank of the true class and the calibration counts, in one read of the probabilities.
//
//   score_hist_kernel<LDS>   persistent: one block of 16 waves per compute unit at most, waves stride over GROUPS of rows.  A wave is cut
//                            into 64 / G segments of G = 2^k lanes, G the power of two that holds C (64 for C >= 64); a segment owns one
//                            row, a lane the classes s, s + G, ... of it.  Up to C = 64 that is a lane per element, and the rows of a group
//                            are consecutive in memory, so a wave's load is one contiguous run; above, it is a row per wave.  Four groups
//                            are loaded before the first is counted (labels, then scores), so that a wave keeps four loads in flight.
//                            The rank of the true class is a wave reduction: one ballot of "this class is ahead of the true one" per
//                            chunk of G classes and the population count of the segment's bits; the largest bin is a xor-shuffle maximum
//                            over the segment.
//     LDS = true             counters are int32 in LDS: hist (2 C bins), then calib (2 bins) and rank_counts (C) while all of it fits
//                            the 160 KiB of a compute unit (C = 1 with many bins does not: those two then count into global memory).
//                            A block's counter cannot pass 2^31: B is an int.  At its end the block adds every non-zero counter to
//                            the int64 arrays with one atomic each.
//     LDS = false            counts go to global memory with 64-bit atomic adds.  A lane counts the same class row after row (up to 64
//                            classes), and scores crowd into few bins (non-targets near 0), so a lane holds its last counter's address
//                            and a run length in registers and issues the add when the address changes: a run of equal bins costs one
//                            atomic, and the hottest addresses get the fewest.  rank_counts and calib take the same route.
//
// Integer counts only: no result depends on the grid or on the order of the atomics.
#include <algorithm>
#include <cstdint>

#include "kws_common.h"

namespace kws {
namespace score {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kUnroll = 4;
constexpr int kMaxLdsBytes = 160 * 1024;          // what one workgroup may declare on gfx950
constexpr int kMinRowsPerBlock = 1024;            // LDS path: a smaller batch takes fewer blocks, each of which flushes its counters

typedef unsigned long long u64;

__device__ __forceinline__ int score_bin(float p, int bins, float fbins)
{
    if (!(p > 0.f)) return 0;
    if (p >= 1.f) return bins - 1;
    return min(bins - 1, (int)(p * fbins));
}

// a run of counts for one global counter, held in registers until the lane counts for another one
struct Run {
    u64 *p = nullptr;
    unsigned n = 0;
    __device__ __forceinline__ void flush()
    {
        if (n) atomicAdd(p, (u64)n);
        n = 0;
    }
    __device__ __forceinline__ void add(u64 *q)
    {
        if (q != p) { flush(); p = q; }
        ++n;
    }
};

template <bool LDS>
__global__ __launch_bounds__(kThreads) void score_hist_kernel(const float *__restrict__ probs, const int32_t *__restrict__ labels, int B,
                                                              int C, int bins, int log_g, u64 *__restrict__ hist, u64 *__restrict__ rank,
                                                              u64 *__restrict__ calib, int aux_lds)
{
    extern __shared__ int lds[];
    const size_t n_hist = (size_t)2 * C * bins;
    const size_t n_lds = LDS ? n_hist + (aux_lds ? (size_t)2 * bins + C : 0) : 0;
    int *const l_calib = lds + n_hist, *const l_rank = l_calib + 2 * bins;      // used when aux_lds only
    if (LDS) {
        for (size_t i = threadIdx.x; i < n_lds; i += kThreads) lds[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << log_g, R = 64 >> log_g;              // lanes per row, rows per wave
    const int s = lane & (G - 1), r = lane >> log_g, shift = r << log_g;
    const u64 seg_mask = G == 64 ? ~0ull : (1ull << G) - 1ull;
    const float fbins = (float)bins;
    const long groups = ((long)B + R - 1) / R, W = (long)gridDim.x * kWaves;
    const bool aux_global = !(LDS && aux_lds);
    Run run_hist, run_rank, run_calib, run_hit;

    for (long g0 = (long)blockIdx.x * kWaves + wave; g0 < groups; g0 += W * kUnroll) {     // wave-uniform
        long row[kUnroll];
        int y[kUnroll];
        float p0[kUnroll], py[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            row[u] = (g0 + u * W) * R + r;                   // a group past the end has row >= B in every lane
            y[u] = row[u] < B ? labels[row[u]] : -1;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool ok = y[u] >= 0 && y[u] < C;           // also false for a row past the end
            const float *const pr = probs + (size_t)(ok ? row[u] : 0) * C;
            p0[u] = ok && s < C ? pr[s] : 0.f;
            py[u] = ok ? pr[y[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (g0 + u * W >= groups) break;                 // wave-uniform
            const bool ok = y[u] >= 0 && y[u] < C;
            const float *const pr = probs + (size_t)(ok ? row[u] : 0) * C;
            int ahead = 0, max_bin = 0;
            bool has_nan = false;
            for (int c0 = 0; c0 < C; c0 += G) {              // wave-uniform: the ballots below are taken by all 64 lanes
                const int c = c0 + s;
                const bool act = ok && c < C;
                const float p = c0 == 0 ? p0[u] : (act ? pr[c] : 0.f);
                const int b = score_bin(p, bins, fbins);
                if (act) {
                    const size_t i = ((size_t)c * 2 + (c == y[u])) * bins + b;
                    if (LDS) atomicAdd(lds + i, 1);
                    else run_hist.add(hist + i);
                    max_bin = max(max_bin, b);
                }
                const u64 m_ahead = __ballot(act && (p > py[u] || (p == py[u] && c < y[u])));
                const u64 m_nan = __ballot(act && p != p);
                ahead += __popcll((m_ahead >> shift) & seg_mask);
                has_nan |= ((m_nan >> shift) & seg_mask) != 0;
            }
            for (int off = G >> 1; off; off >>= 1) max_bin = max(max_bin, __shfl_xor(max_bin, off));
            if (ok && s == 0) {
                const int rk = has_nan ? C - 1 : ahead;       // ahead <= C - 1: the true class is never ahead of itself
                if (rank) {
                    if (aux_global) run_rank.add(rank + rk);
                    else atomicAdd(l_rank + rk, 1);
                }
                if (calib) {
                    if (aux_global) {
                        run_calib.add(calib + max_bin);
                        if (rk == 0) run_hit.add(calib + bins + max_bin);
                    } else {
                        atomicAdd(l_calib + max_bin, 1);
                        if (rk == 0) atomicAdd(l_calib + bins + max_bin, 1);
                    }
                }
            }
        }
    }

    run_hist.flush();
    run_rank.flush();
    run_calib.flush();
    run_hit.flush();
    if (LDS) {
        __syncthreads();
        for (size_t i = threadIdx.x; i < n_hist; i += kThreads)
            if (const int v = lds[i]) atomicAdd(hist + i, (u64)v);
        if (aux_lds) {
            if (calib)
                for (int i = threadIdx.x; i < 2 * bins; i += kThreads)
                    if (const int v = l_calib[i]) atomicAdd(calib + i, (u64)v);
            if (rank)
                for (int i = threadIdx.x; i < C; i += kThreads)
                    if (const int v = l_rank[i]) atomicAdd(rank + i, (u64)v);
        }
    }
}

}  // namespace score
}  // namespace kws

using namespace kws;
using namespace kws::score;

extern "C" {

int kws_score_hist_uses_lds(int C, int bins)
{
    return C >= 1 && bins >= 2 && (int64_t)2 * C * bins * (int64_t)sizeof(int32_t) <= (int64_t)KWS_SCORE_LDS_BUDGET;
}

int kws_score_hist(const float *probs, const int32_t *labels, int B, int C, int bins, int64_t *hist, int64_t *rank_counts,
                   int64_t *calib, void *stream)
{
    if (!probs || !labels || !hist) return fail(KWS_ERR_INVALID, "null argument");
    if (B < 0 || C < 1 || bins < 2) return fail(KWS_ERR_INVALID, "bad shape: B %d, C %d, bins %d (B >= 0, C >= 1, bins >= 2)", B, C, bins);
    if (B == 0) return KWS_OK;
    int log_g = 1;                                       // segments of at least two lanes
    while (log_g < 6 && (1 << log_g) < C) ++log_g;
    const int R = 64 >> log_g;
    const long groups = ((long)B + R - 1) / R;
    const long want = (groups + (long)kWaves * kUnroll - 1) / ((long)kWaves * kUnroll);
    hipStream_t s = static_cast<hipStream_t>(stream);
    u64 *const h = reinterpret_cast<u64 *>(hist), *const rk = reinterpret_cast<u64 *>(rank_counts), *const cal = reinterpret_cast<u64 *>(calib);
    if (kws_score_hist_uses_lds(C, bins)) {
        const size_t hist_bytes = (size_t)2 * C * bins * sizeof(int32_t), aux_bytes = ((size_t)2 * bins + C) * sizeof(int32_t);
        const int aux_lds = hist_bytes + aux_bytes <= (size_t)kMaxLdsBytes;
        const size_t smem = hist_bytes + (aux_lds ? aux_bytes : 0);
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&score_hist_kernel<true>), (int)smem)) return rc;
        const long by_rows = ((long)B + kMinRowsPerBlock - 1) / kMinRowsPerBlock;
        const int blocks = (int)std::max(1L, std::min((long)device_cus(), std::min(want, by_rows)));
        KWS_LAUNCH("score_hist_kernel", score_hist_kernel<true>, dim3(blocks), dim3(kThreads), smem, s, probs, labels, B, C, bins, log_g, h,
                   rk, cal, aux_lds);
    } else {
        const int blocks = (int)std::max(1L, std::min((long)device_cus(), want));
        KWS_LAUNCH("score_hist_kernel", score_hist_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, probs, labels, B, C, bins, log_g, h, rk,
                   cal, 0);
    }
    KWS_LAUNCH_CHECK("score_hist_kernel");
    return KWS_OK;
}

}  // extern "C"
