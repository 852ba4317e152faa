// csrc/kws_knn.hip -- exact k-nearest-neighbour search over embeddings (include/kws.h): kws_rows_normalize,
// kws_knn, kws_knn_vote.
//
// knn_kernel: a 256-thread block owns a tile of 128 queries and one slice of the reference rows.  Wave w holds queries 32 w .. 32 w + 31
// as the B operand of v_mfma_f32_32x32x2_f32 in REGISTERS for the whole launch (E / 2 values per lane), the block walks its slice in
// tiles of 32 reference rows that are staged in LDS (loads of the next tile are issued before the current tile's products and stored
// behind them), and every wave multiplies the tile into one 32 x 32 accumulator: the reference rows are the A operand, so a lane
// ends up with the scores of ONE query (column lane & 31) against 16 reference rows.  Two blocks fit a compute unit (registers, and
// LDS up to k = 32), so one wave's selection runs under another's products.  An MFMA of this kind is bit for bit the
// fmaf chain over its k index, and the k index runs over the columns in ascending order: a score depends on its two rows only.
// Selection: every query keeps its k best (key, index) pairs sorted in LDS; a lane compares its 16 candidates with the query's
// current k-th best and only the few that beat it are inserted.  The two lanes that share a query (lane, lane + 32) insert one
// after the other.  With more than one slice the lists go to the workspace and knn_merge_kernel merges them by the same total order
// (larger key first, then the lower index), so the result does not depend on the number of slices: no atomics anywhere.
// Inside the kernels a score is a KEY that is better when larger: the dot product, or minus the squared distance.
#include <climits>
#include <cmath>

#include "kws_common.h"

namespace kws {

namespace {

typedef float knn_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKnnThreads = 256;
constexpr int kKnnTQ = 128;                // queries of a block: 32 per wave
constexpr int kKnnTN = 32;                 // reference rows of a tile: one 32 x 32 MFMA tile per wave
constexpr int kKnnMaxE = 128;
constexpr int kKnnGroups = kKnnMaxE / 8;   // a group: 8 columns = 4 MFMAs, one 128-bit LDS read per operand
constexpr int kKnnMaxSlices = 1024;
constexpr int kKnnEmpty = INT_MAX;         // index of an empty list slot: any real candidate of key -inf still beats it
constexpr int kKnnVoteThreads = 64;

inline int knn_ep(int E) { return (E + 7) / 8 * 8; }
inline int knn_stride(int E) { return knn_ep(E) + 4; }         // floats of a tile row: 16-byte aligned, consecutive rows 4 banks apart
inline int knn_kstride(int k) { return k | 1; }               // odd: the lists of a wave's queries fall into different banks
inline size_t knn_lds_bytes(int E, int k)
{
    return sizeof(float) * ((size_t)2 * kKnnTN * knn_stride(E) + 2 * kKnnTN + (size_t)2 * kKnnTQ * knn_kstride(k));
}
inline int64_t knn_default_slices(int64_t Q, int64_t N)
{
    // enough blocks for two per compute unit of the 256, but at least 8 tiles (256 rows) of work per slice
    const int64_t qt = (Q + kKnnTQ - 1) / kKnnTQ, tiles = (N + kKnnTN - 1) / kKnnTN;
    if (qt >= 256 || qt < 1) return 1;
    int64_t s = (512 + qt - 1) / qt;
    s = std::min<int64_t>(s, std::max<int64_t>(1, tiles / 8));
    return std::min<int64_t>(s, kKnnMaxSlices);
}

__device__ __forceinline__ bool knn_better(float k1, int i1, float k2, int i2) { return k1 > k2 || (k1 == k2 && i1 < i2); }

// inserts (key, idx) into the sorted list of one query; the caller has seen it beat some earlier k-th best, the list may have moved on
__device__ __forceinline__ void knn_insert(volatile float *lk, volatile int *li, int k, float key, int idx)
{
    if (!knn_better(key, idx, lk[k - 1], li[k - 1])) return;
    int p = k - 1;
    while (p > 0) {
        const float pk = lk[p - 1];
        const int pi = li[p - 1];
        if (!knn_better(key, idx, pk, pi)) break;
        lk[p] = pk;
        li[p] = pi;
        --p;
    }
    lk[p] = key;
    li[p] = idx;
}

// element r (a runtime value) of an accumulator: 15 selects instead of a branch per element
__device__ __forceinline__ float knn_pick(const knn_f32x16 &a, int r)
{
    float v = a[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) v = r == i ? a[i] : v;
    return v;
}

template <bool L2>
__global__ __launch_bounds__(kKnnThreads, 2) void knn_kernel(const float *__restrict__ queries, long Q, const float *__restrict__ refs, int N, int E,
                                                              int k, const int32_t *__restrict__ exclude, int tiles_per_slice, int slices,
                                                              int32_t *__restrict__ out_idx, float *__restrict__ out_score,
                                                              float *__restrict__ ws_key, int32_t *__restrict__ ws_idx)
{
#pragma clang fp contract(off)
    extern __shared__ float4 knn_smem[];
    const int stride = (E + 7) / 8 * 8 + 4, ks = k | 1;
    float *tile = reinterpret_cast<float *>(knn_smem);                 // [2][kKnnTN][stride], columns permuted inside groups of 8
    float *sh_rr = tile + 2 * kKnnTN * stride;                        // [2][kKnnTN]: r.r of the tile's rows (L2)
    float *lkey = sh_rr + 2 * kKnnTN;                                  // [kKnnTQ][ks]
    int *lidx = reinterpret_cast<int *>(lkey + kKnnTQ * ks);          // [kKnnTQ][ks]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, j = lane & 31;
    const int ntiles = (int)(((long)N + kKnnTN - 1) / kKnnTN);
    const int slice = blockIdx.y;
    const long first_l = (long)slice * tiles_per_slice;
    const int first = (int)(first_l < ntiles ? first_l : ntiles);
    const int last = (int)(first_l + tiles_per_slice < ntiles ? first_l + tiles_per_slice : ntiles);
    const int ng = (E + 7) / 8, q4 = E / 4;
    const int qloc = wave * 32 + j;                                    // this lane's query inside the block
    const long gq = (long)blockIdx.x * kKnnTQ + qloc;
    const bool qlive = gq < Q;

    // the lists of this wave's queries, and zeros in both tiles (the padding columns of E % 8 == 4 are never written again)
    for (int p = lane; p < 32 * ks; p += 64) {
        lkey[wave * 32 * ks + p] = -INFINITY;
        lidx[wave * 32 * ks + p] = kKnnEmpty;
    }
    for (int p = t; p < 2 * kKnnTN * stride; p += kKnnThreads) tile[p] = 0.f;

    // the query operand: step i of group g multiplies column 8 g + 2 i + h; q.q is the same ascending chain as every other product
    float4 qf[kKnnGroups];
    float qq = 0.f;
#pragma unroll
    for (int g = 0; g < kKnnGroups; ++g) {
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (qlive && 8 * g < E) lo = *reinterpret_cast<const float4 *>(queries + gq * E + 8 * g);
        if (qlive && 8 * g + 4 < E) hi = *reinterpret_cast<const float4 *>(queries + gq * E + 8 * g + 4);
        qf[g] = h ? make_float4(lo.y, lo.w, hi.y, hi.w) : make_float4(lo.x, lo.z, hi.x, hi.z);
        if (L2) {
            qq = fmaf(lo.x, lo.x, qq); qq = fmaf(lo.y, lo.y, qq); qq = fmaf(lo.z, lo.z, qq); qq = fmaf(lo.w, lo.w, qq);
            qq = fmaf(hi.x, hi.x, qq); qq = fmaf(hi.y, hi.y, qq); qq = fmaf(hi.z, hi.z, qq); qq = fmaf(hi.w, hi.w, qq);
        }
    }
    const int excl = (exclude && qlive) ? exclude[gq] : -1;

    // staging of one tile: a row's E / 4 float4 are dealt to a power-of-two run of threads (no division in the loop), at most 4 per
    // thread; column 4 c + i of a row goes to position 8 (c / 2) + 4 (i & 1) + 2 (c & 1) + (i >> 1)
    int q4s = 0;
    while ((1 << q4s) < q4) ++q4s;
    float4 px[4];
    auto fetch = [&](int tl) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = t + p * kKnnThreads, r = i >> q4s, c = i & ((1 << q4s) - 1);
            const long row = (long)tl * kKnnTN + r;
            px[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < kKnnTN && c < q4 && row < N) px[p] = *reinterpret_cast<const float4 *>(refs + row * E + 4 * c);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = t + p * kKnnThreads, r = i >> q4s, c = i & ((1 << q4s) - 1);
            if (r < kKnnTN && c < q4) {
                float *d = tile + (buf * kKnnTN + r) * stride + 8 * (c >> 1) + 2 * (c & 1);
                *reinterpret_cast<float2 *>(d) = make_float2(px[p].x, px[p].z);
                *reinterpret_cast<float2 *>(d + 4) = make_float2(px[p].y, px[p].w);
            }
        }
    };

    __syncthreads();
    if (first < last) { fetch(first); stash(0); }
    __syncthreads();

    volatile float *my_key = lkey + qloc * ks;
    volatile int *my_idx = lidx + qloc * ks;
    int buf = 0;
    for (int tl = first; tl < last; ++tl, buf ^= 1) {
        const bool more = tl + 1 < last;
        if (more) fetch(tl + 1);
        const float *tb = tile + buf * kKnnTN * stride;
        if (L2 && lane < 8) {                                           // r.r of 8 rows per wave; the zero padding adds nothing
            const float *row = tb + (wave * 8 + lane) * stride;
            float rr = 0.f;
            for (int g = 0; g < ng; ++g) {
                const float4 ev = *reinterpret_cast<const float4 *>(row + 8 * g), od = *reinterpret_cast<const float4 *>(row + 8 * g + 4);
                rr = fmaf(ev.x, ev.x, rr); rr = fmaf(od.x, od.x, rr); rr = fmaf(ev.y, ev.y, rr); rr = fmaf(od.y, od.y, rr);
                rr = fmaf(ev.z, ev.z, rr); rr = fmaf(od.z, od.z, rr); rr = fmaf(ev.w, ev.w, rr); rr = fmaf(od.w, od.w, rr);
            }
            sh_rr[buf * kKnnTN + wave * 8 + lane] = rr;
        }
        knn_f32x16 acc = {};
        const float *ap = tb + j * stride + 4 * h;
#pragma unroll
        for (int g = 0; g < kKnnGroups; ++g) {
            if (g < ng) {
                const float4 a = *reinterpret_cast<const float4 *>(ap + 8 * g);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qf[g].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qf[g].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qf[g].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qf[g].w, acc, 0, 0, 0);
            }
        }
        if (L2) __syncthreads();                                        // sh_rr of the other waves' rows

        // element r of the accumulator is the tile's row (r & 3) + 8 (r >> 2) + 4 h; its key, and whether it is a candidate at all
        const long row0 = (long)tl * kKnnTN + 4 * h;
        auto key_of = [&](float s, int loc) {
            float kv = s;
            if (L2) {
                const float d = (qq + sh_rr[buf * kKnnTN + loc + 4 * h]) - 2.f * s;
                kv = d == d ? -fmaxf(0.f, d) : d;                        // fmaxf would turn a NaN into the best distance
            }
            return kv == kv ? kv : -INFINITY;                            // a NaN ranks last
        };
        // which of the 16 beat the query's k-th best as it stands
        const float thr_k = my_key[k - 1];
        const int thr_i = my_idx[k - 1];
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int loc = (r & 3) + 8 * (r >> 2);
            const float kv = key_of(acc[r], loc);
            const long gl = row0 + loc;                                  // rows past N are zeros in the tile and no candidates
            const int gi = gl < N ? (int)gl : -1;
            const bool ok = qlive && gi >= 0 && gi != excl && knn_better(kv, gi, thr_k, thr_i);
            mask |= ok ? (1u << r) : 0u;
        }
        // the few that did: every lane inserts its next one, the two lanes of a query one after the other (knn_insert looks at the
        // list as it is by then)
        while (__any(mask != 0)) {
            const bool want = mask != 0;
            const int r = want ? __ffs(mask) - 1 : 0, loc = (r & 3) + 8 * (r >> 2);
            const float kv = key_of(knn_pick(acc, r), loc);
            const int gi = (int)(row0 + loc);
            mask &= mask - 1;
#pragma unroll 1
            for (int hh = 0; hh < 2; ++hh) {
                if (want && h == hh) knn_insert(my_key, my_idx, k, kv, gi);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
    }

    // the lists of this wave's queries: the result itself, or one slice's share of it
    for (int p = lane; p < 32 * k; p += 64) {
        const int ql = p / k, pos = p - ql * k;
        const long g = (long)blockIdx.x * kKnnTQ + wave * 32 + ql;
        if (g >= Q) continue;
        const float kv = lkey[(wave * 32 + ql) * ks + pos];
        const int iv = lidx[(wave * 32 + ql) * ks + pos];
        if (slices == 1) {
            out_idx[g * k + pos] = iv == kKnnEmpty ? -1 : iv;
            out_score[g * k + pos] = L2 ? -kv : kv;
        } else {
            const long o = ((long)slice * Q + g) * k + pos;
            ws_key[o] = kv;
            ws_idx[o] = iv;
        }
    }
}

// one wave per query: k rounds, each takes the best head of the query's `slices` sorted lists
__global__ __launch_bounds__(64) void knn_merge_kernel(const float *__restrict__ ws_key, const int32_t *__restrict__ ws_idx, long Q, int k,
                                                        int slices, int l2, int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    __shared__ unsigned char head[kKnnMaxSlices];
    const int lane = threadIdx.x;
    const long q = blockIdx.x;
    for (int s = lane; s < slices; s += 64) head[s] = 0;                 // a lane touches the heads of its own slices only
    for (int pos = 0; pos < k; ++pos) {
        float bk = -INFINITY;
        int bi = kKnnEmpty, bs = -1;
        for (int s = lane; s < slices; s += 64) {
            const int hp = head[s];
            if (hp >= k) continue;
            const long o = ((long)s * Q + q) * k + hp;
            const float kv = ws_key[o];
            const int iv = ws_idx[o];
            if (knn_better(kv, iv, bk, bi)) { bk = kv; bi = iv; bs = s; }
        }
        float wk = bk;
        int wi = bi;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ok = __shfl_xor(wk, o, 64);
            const int oi = __shfl_xor(wi, o, 64);
            if (knn_better(ok, oi, wk, wi)) { wk = ok; wi = oi; }
        }
        if (bs >= 0 && wi == bi) head[bs] = (unsigned char)(head[bs] + 1);        // real indices are distinct: one winner
        if (lane == 0) {
            out_idx[q * k + pos] = wi == kKnnEmpty ? -1 : wi;
            out_score[q * k + pos] = l2 ? -wk : wk;
        }
    }
}

// 32 lanes per row, 8 rows per block; the sum of squares in double, in a fixed order
__global__ __launch_bounds__(256) void rows_normalize_kernel(const float *x, long N, int E, float *out, float *norms)
{
    const int t = threadIdx.x, c = t & 31;
    const long row = (long)blockIdx.x * 8 + (t >> 5);
    const bool on = row < N && 4 * c < E;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) v = *reinterpret_cast<const float4 *>(x + row * E + 4 * c);
    double ss = (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 32);
    const double nd = sqrt(ss);
    if (on) {
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nd > 0.0) u = make_float4((float)(v.x / nd), (float)(v.y / nd), (float)(v.z / nd), (float)(v.w / nd));
        *reinterpret_cast<float4 *>(out + row * E + 4 * c) = u;
    }
    if (norms && c == 0 && row < N) norms[row] = (float)nd;
}

// one thread per query; the neighbours' labels and weights of the block's queries in LDS
__global__ __launch_bounds__(kKnnVoteThreads) void knn_vote_kernel(const int32_t *__restrict__ idx, const float *__restrict__ score, long Q, int k,
                                                                   const int32_t *__restrict__ labels, int N, int C, int weighted,
                                                                   const int32_t *__restrict__ own_labels, int32_t *__restrict__ pred,
                                                                   float *__restrict__ support, float *__restrict__ own)
{
    __shared__ int lab[kKnnVoteThreads][KWS_KNN_MAX_K + 1];
    __shared__ float wt[kKnnVoteThreads][KWS_KNN_MAX_K + 1];
    const int t = threadIdx.x;
    const long q = (long)blockIdx.x * kKnnVoteThreads + t;
    if (q >= Q) return;
    float total = 0.f;
    for (int a = 0; a < k; ++a) {
        const int i = idx[q * k + a];
        int c = -1;
        float w = 0.f;
        if (i >= 0 && i < N) {                                          // an index outside the reference rows casts no vote
            c = labels[i];
            if (c < 0 || c >= C) c = -1;
            else w = weighted ? fmaxf(score[q * k + a], 0.f) : 1.f;
            if (!(w == w)) w = 0.f;
        }
        lab[t][a] = c;
        wt[t][a] = c >= 0 ? w : 0.f;
        total += wt[t][a];
    }
    int best_c = -1;
    float best = 0.f;
    for (int a = 0; a < k; ++a) {
        const int c = lab[t][a];
        if (c < 0) continue;
        float tot = 0.f;
        for (int b = 0; b < k; ++b) tot += lab[t][b] == c ? wt[t][b] : 0.f;
        if (tot > best || (tot == best && best_c >= 0 && c < best_c)) { best = tot; best_c = c; }
    }
    const bool any = total > 0.f && best_c >= 0;
    pred[q] = any ? best_c : -1;
    support[q] = any ? best / total : 0.f;
    if (own) {
        const int oc = own_labels[q];
        float tot = 0.f;
        for (int b = 0; b < k; ++b) tot += (oc >= 0 && lab[t][b] == oc) ? wt[t][b] : 0.f;
        own[q] = any ? tot / total : 0.f;
    }
}

int knn_check_shape(const char *who, int64_t Q, int64_t N, int E, int k, int slices)
{
    if (E < 4 || E > kKnnMaxE || E % 4) return fail(KWS_ERR_INVALID, "%s: E = %d is not a multiple of 4 in 4 .. %d", who, E, kKnnMaxE);
    if (k < 1 || k > KWS_KNN_MAX_K) return fail(KWS_ERR_INVALID, "%s: k = %d outside 1 .. %d", who, k, KWS_KNN_MAX_K);
    if (Q < 0) return fail(KWS_ERR_INVALID, "%s: Q = %lld queries", who, (long long)Q);
    if (N < 1 || N > (int64_t)INT_MAX) return fail(KWS_ERR_INVALID, "%s: N = %lld reference rows outside 1 .. 2^31 - 1", who, (long long)N);
    if (slices < 0 || slices > kKnnMaxSlices) return fail(KWS_ERR_INVALID, "%s: slices = %d outside 0 .. %d", who, slices, kKnnMaxSlices);
    if ((Q + kKnnTQ - 1) / kKnnTQ > (int64_t)INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "%s: Q = %lld is more than one launch takes", who, (long long)Q);
    return KWS_OK;
}

inline int64_t knn_ws_bytes(int64_t Q, int k, int64_t slices) { return slices > 1 ? (slices * Q * k * 8 + 255) / 256 * 256 : 0; }

}  // namespace

}  // namespace kws

using namespace kws;

extern "C" {

int kws_rows_normalize(const float *x, int64_t N, int E, float *out, float *norms, void *stream)
{
    if (E < 4 || E > kKnnMaxE || E % 4) return fail(KWS_ERR_INVALID, "rows normalize: E = %d is not a multiple of 4 in 4 .. %d", E, kKnnMaxE);
    if (N < 0) return fail(KWS_ERR_INVALID, "rows normalize: N = %lld rows", (long long)N);
    if (!x || !out) return fail(KWS_ERR_INVALID, "rows normalize: null argument");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) return fail(KWS_ERR_INVALID, "rows normalize: x and out must be 16-byte aligned");
    if ((N + 7) / 8 > (int64_t)INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "rows normalize: N = %lld is more than one launch takes", (long long)N);
    if (N == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    KWS_LAUNCH("rows_normalize_kernel", rows_normalize_kernel, dim3((unsigned)((N + 7) / 8)), dim3(256), 0, s, x, (long)N, E, out, norms);
    KWS_LAUNCH_CHECK("rows_normalize_kernel");
    return KWS_OK;
}

int64_t kws_knn_workspace_bytes(int64_t Q, int64_t N, int E, int k, int slices)
{
    if (int rc = knn_check_shape("knn workspace", Q, N, E, k, slices)) return rc;
    return knn_ws_bytes(Q, k, slices ? slices : knn_default_slices(Q, N));
}

int kws_knn(const float *queries, int64_t Q, const float *refs, int64_t N, int E, int metric, int k, const int32_t *exclude, int slices,
            int32_t *idx, float *score, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = knn_check_shape("knn", Q, N, E, k, slices)) return rc;
    if (metric != KWS_KNN_DOT && metric != KWS_KNN_L2) return fail(KWS_ERR_INVALID, "knn: metric = %d (KWS_KNN_DOT or KWS_KNN_L2)", metric);
    if (!queries || !refs || !idx || !score) return fail(KWS_ERR_INVALID, "knn: null argument");
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(refs)) & 15) return fail(KWS_ERR_INVALID, "knn: queries and refs must be 16-byte aligned");
    if (Q == 0) return KWS_OK;
    const int ns = (int)(slices ? slices : knn_default_slices(Q, N));
    const size_t need = (size_t)knn_ws_bytes(Q, k, ns);
    if (need && (!ws || ws_bytes < need))
        return fail(KWS_ERR_WORKSPACE, "knn: %d slices need a workspace of %zu bytes (kws_knn_workspace_bytes), got %zu", ns, need, ws ? ws_bytes : (size_t)0);
    if (need && (reinterpret_cast<uintptr_t>(ws) & 3)) return fail(KWS_ERR_INVALID, "knn: the workspace must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t tiles = (N + kKnnTN - 1) / kKnnTN;
    const int tps = (int)((tiles + ns - 1) / ns);
    const int lds = (int)knn_lds_bytes(E, k);
    float *ws_key = static_cast<float *>(ws);
    int32_t *ws_idx = need ? reinterpret_cast<int32_t *>(ws_key + (size_t)ns * Q * k) : nullptr;
    const dim3 grid((unsigned)((Q + kKnnTQ - 1) / kKnnTQ), (unsigned)ns);
    if (metric == KWS_KNN_L2) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&knn_kernel<true>), lds)) return rc;
        KWS_LAUNCH("knn_kernel", knn_kernel<true>, grid, dim3(kKnnThreads), (size_t)lds, s, queries, (long)Q, refs, (int)N, E, k, exclude, tps, ns,
                   idx, score, ws_key, ws_idx);
    } else {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&knn_kernel<false>), lds)) return rc;
        KWS_LAUNCH("knn_kernel", knn_kernel<false>, grid, dim3(kKnnThreads), (size_t)lds, s, queries, (long)Q, refs, (int)N, E, k, exclude, tps, ns,
                   idx, score, ws_key, ws_idx);
    }
    KWS_LAUNCH_CHECK("knn_kernel");
    if (ns > 1) {
        KWS_LAUNCH("knn_merge_kernel", knn_merge_kernel, dim3((unsigned)Q), dim3(64), 0, s, ws_key, ws_idx, (long)Q, k, ns, metric == KWS_KNN_L2 ? 1 : 0,
                   idx, score);
        KWS_LAUNCH_CHECK("knn_merge_kernel");
    }
    return KWS_OK;
}

int kws_knn_vote(const int32_t *idx, const float *score, int64_t Q, int k, const int32_t *labels, int64_t N, int C, int weighted,
                 const int32_t *own_labels, int32_t *pred, float *support, float *own, void *stream)
{
    if (k < 1 || k > KWS_KNN_MAX_K) return fail(KWS_ERR_INVALID, "knn vote: k = %d outside 1 .. %d", k, KWS_KNN_MAX_K);
    if (C < 2 || C > 1024) return fail(KWS_ERR_INVALID, "knn vote: C = %d classes outside 2 .. 1024", C);
    if (Q < 0) return fail(KWS_ERR_INVALID, "knn vote: Q = %lld queries", (long long)Q);
    if (N < 1 || N > (int64_t)INT_MAX) return fail(KWS_ERR_INVALID, "knn vote: N = %lld reference rows outside 1 .. 2^31 - 1", (long long)N);
    if (!idx || !labels || !pred || !support) return fail(KWS_ERR_INVALID, "knn vote: null argument");
    if (weighted && !score) return fail(KWS_ERR_INVALID, "knn vote: weighted votes need the scores");
    if ((own == nullptr) != (own_labels == nullptr)) return fail(KWS_ERR_INVALID, "knn vote: own and own_labels come together or not at all");
    if ((Q + kKnnVoteThreads - 1) / kKnnVoteThreads > (int64_t)INT_MAX) return fail(KWS_ERR_UNSUPPORTED, "knn vote: Q = %lld is more than one launch takes", (long long)Q);
    if (Q == 0) return KWS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    KWS_LAUNCH("knn_vote_kernel", knn_vote_kernel, dim3((unsigned)((Q + kKnnVoteThreads - 1) / kKnnVoteThreads)), dim3(kKnnVoteThreads), 0, s, idx, score,
               (long)Q, k, labels, (int)N, C, weighted, own_labels, pred, support, own);
    KWS_LAUNCH_CHECK("knn_vote_kernel");
    return KWS_OK;
}

}  // extern "C"
