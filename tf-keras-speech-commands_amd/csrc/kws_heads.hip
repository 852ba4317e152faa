// csrc/kws_heads.hip -- kws_heads_apply: every row of a batch of embeddings through the Dense(E -> C_h, softmax) head that row names, out of
// a bank of heads resident on the device (include/kws.h).
//
// One 256-thread block per tile of KWS_HEADS_TILE_ROWS = 16 consecutive output rows, four rows per wave.
//   resolve   thread j < 16 walks row j's indirections (rows, key, head_of_key, head_classes, head_offset) and clamps: a row that leads
//             outside anything gets C = 0 and is written as zeros / -1 without another read.
//   stage     the tile's embedding rows go to LDS (float4, rows padded by 4 floats so that the rows a wave reads together start on
//             different banks); invalid rows are zeros.
//   route     every thread compares the tile's head ids (16 broadcast LDS reads, the same answer in every wave).  All equal and the head
//             within kStageFloats: the head is copied to LDS once and the chains below read it there (the "run" route, evaluation:
//             consecutive rows of one fold).  Otherwise every row reads its own head from memory (serving: a head per row, coalesced
//             over the classes, served by L2 when heads repeat).
//   chain     lane = (row of the wave, class): with CP = the next power of two >= Cmax (at most 64) a wave takes 64 / CP of its four rows
//             at a time, so a 12-class bank keeps all 64 lanes busy; past 64 classes a lane owns c, c + 64, .. (KC of them).  A lane
//             runs the ONE chain of the contract for each of its classes -- acc = b; acc = fma(x_e, W[e][c], acc), e ascending -- so
//             the bits cannot depend on the route, the tile or CP.  Contraction is off and the multiply-adds are spelled out.
//   softmax   max and arg-max (tie: lower class) by xor-shuffles inside the CP-lane group, exact in any order; the sum is taken by
//             every lane of the group over c = 0, 1, .. in that order (shuffle from the owner), so it has one order too; expf and
//             the division are the precise ones (no fast-math flag in this library's build).
#include <cmath>

#include "kws_common.h"

namespace kws {

namespace {

constexpr int kHbThreads = 256;
constexpr int kHbRows = KWS_HEADS_TILE_ROWS;
constexpr int kHbWaveRows = kHbRows / (kHbThreads / 64);       // rows of a tile per wave
constexpr int kHbMaxE = 128;
constexpr int kHbXStride = kHbMaxE + 4;                         // floats between two staged rows
constexpr int kStageFloats = 4096;                              // a head up to 16 KiB is staged for a run (E = 128: up to 31 classes)
static_assert(kHbRows == 16 && kHbWaveRows == 4, "the tile is four waves of four rows");

struct HbShape {
    int64_t N, key_stride, K, R, weights_count;
    int E, H, Cmax, cp_log2;
};

// the chains of one lane: its row's embedding from LDS, the head from `w` (LDS or memory), KC classes c0 + 64 k
template <int KC>
__device__ __forceinline__ void hb_chain(const float *__restrict__ xr, const float *__restrict__ w, int E, int C, int c0, float (&acc)[KC])
{
#pragma clang fp contract(off)
    bool on[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        on[k] = c0 + 64 * k < C;
        acc[k] = on[k] ? w[E * C + c0 + 64 * k] : 0.f;
    }
#pragma unroll 4
    for (int e = 0; e < E; e += 4) {
        const float4 xv = *reinterpret_cast<const float4 *>(xr + e);
        const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const float wv = on[k] ? w[(e + u) * C + c0 + 64 * k] : 0.f;
                acc[k] = fmaf(x4[u], wv, acc[k]);
            }
    }
}

template <int KC>
__global__ __launch_bounds__(kHbThreads) void heads_apply_kernel(const float *__restrict__ emb, const int32_t *__restrict__ rows,
                                                                  const int32_t *__restrict__ key, const int32_t *__restrict__ head_of_key,
                                                                  const float *__restrict__ weights, const int64_t *__restrict__ head_offset,
                                                                  const int32_t *__restrict__ head_classes, HbShape sh,
                                                                  float *__restrict__ logits, float *__restrict__ probs,
                                                                  int32_t *__restrict__ pred)
{
#pragma clang fp contract(off)
    __shared__ __align__(16) float sx[kHbRows * kHbXStride];
    __shared__ float sw[kStageFloats];
    __shared__ int64_t s_src[kHbRows], s_off[kHbRows];
    __shared__ int s_head[kHbRows], s_cls[kHbRows];
    const int t = threadIdx.x, E = sh.E, Cmax = sh.Cmax;
    const int64_t r0 = (int64_t)blockIdx.x * kHbRows;
    const int cnt = (int)(sh.R - r0 < kHbRows ? sh.R - r0 : kHbRows);

    if (t < kHbRows) {
        int64_t src = -1, off = 0;
        int head = -1, cls = 0;
        if (t < cnt) {
            const int64_t r = r0 + t;
            src = rows ? (int64_t)rows[r] : r;
            int64_t h = key[r * sh.key_stride];
            if (head_of_key) h = (h >= 0 && h < sh.K) ? (int64_t)head_of_key[h] : -1;
            if (src >= 0 && src < sh.N && h >= 0 && h < sh.H) {
                const int c = head_classes[h];
                const int64_t o = head_offset[h];
                if (c >= 2 && c <= Cmax && o >= 0 && o <= sh.weights_count - (int64_t)(E + 1) * c) { head = (int)h; cls = c; off = o; }
            }
        }
        s_src[t] = src;
        s_off[t] = off;
        s_head[t] = head;
        s_cls[t] = cls;                                      // 0: the row is written as zeros / -1 and reads nothing more
    }
    __syncthreads();

    const int q4 = E / 4;
    for (int i = t; i < kHbRows * q4; i += kHbThreads) {
        const int j = i / q4, col = i - j * q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s_cls[j]) v = *reinterpret_cast<const float4 *>(emb + s_src[j] * E + 4 * col);
        *reinterpret_cast<float4 *>(&sx[j * kHbXStride + 4 * col]) = v;
    }
    // a run: every row of the tile names the same valid head, and that head fits the staging buffer (the same in every thread)
    const int C0 = s_cls[0], h0 = s_head[0];
    bool run = cnt >= 2 && C0 > 0 && (E + 1) * C0 <= kStageFloats;
    for (int j = 1; j < cnt; ++j) run = run && s_head[j] == h0;
    if (run) {
        const float *w0 = weights + s_off[0];
        for (int i = t; i < (E + 1) * C0; i += kHbThreads) sw[i] = w0[i];
    }
    __syncthreads();

    const int wave = t >> 6, lane = t & 63;
    if (wave * kHbWaveRows >= cnt) return;                   // the whole wave: nothing below is a block-wide barrier
    const int cp = 1 << sh.cp_log2;                          // lanes per row; KC > 1 comes with cp = 64
    const int rpw = 64 / cp < kHbWaveRows ? 64 / cp : kHbWaveRows;          // rows of the wave in flight together
    const int sub = lane >> sh.cp_log2, c0 = lane & (cp - 1), gbase = lane & ~(cp - 1);
    for (int pass = 0; pass < kHbWaveRows / rpw; ++pass) {
        const int j = wave * kHbWaveRows + pass * rpw + sub;
        const bool mine = sub < rpw && j < cnt;              // this lane works for a row of the tile
        const int jj = mine ? j : 0;
        const int C = mine ? s_cls[jj] : 0;
        float acc[KC];
        if (run) hb_chain<KC>(sx + jj * kHbXStride, sw, E, C, c0, acc);
        else hb_chain<KC>(sx + jj * kHbXStride, weights + s_off[jj], E, C, c0, acc);

        // max and arg-max of the row: first inside the lane (ascending c, strict >), then across the group's lanes
        float m = -INFINITY;
        int am = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (c0 + 64 * k < C && acc[k] > m) { m = acc[k]; am = c0 + 64 * k; }
        for (int o = cp >> 1; o >= 1; o >>= 1) {
            const float om = __shfl_xor(m, o);
            const int oa = __shfl_xor(am, o);
            if (om > m || (om == m && oa < am)) { m = om; am = oa; }
        }
        float ev[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) ev[k] = c0 + 64 * k < C ? expf(acc[k] - m) : 0.f;
        // the sum over c ascending, by every lane of the group alike; classes past C hold +0, which changes no partial sum
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k)
            for (int l = 0; l < cp && 64 * k + l < Cmax; ++l) sum += __shfl(ev[k], gbase + l);
        if (mine) {
            const int64_t r = r0 + j;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int c = c0 + 64 * k;
                if (c < Cmax) {
                    const bool on = c < C;
                    if (logits) logits[r * Cmax + c] = on ? acc[k] : 0.f;
                    if (probs) probs[r * Cmax + c] = on ? ev[k] / sum : 0.f;
                }
            }
            if (pred && c0 == 0) pred[r] = C > 0 ? am : -1;
        }
    }
}

template <int KC>
int launch_heads_apply(const float *emb, const int32_t *rows, const int32_t *key, const int32_t *head_of_key, const float *weights,
                       const int64_t *head_offset, const int32_t *head_classes, const HbShape &sh, float *logits, float *probs, int32_t *pred,
                       hipStream_t s)
{
    const unsigned grid = (unsigned)((sh.R + kHbRows - 1) / kHbRows);
    KWS_LAUNCH("heads_apply_kernel", heads_apply_kernel<KC>, dim3(grid), dim3(kHbThreads), 0, s, emb, rows, key, head_of_key, weights,
               head_offset, head_classes, sh, logits, probs, pred);
    KWS_LAUNCH_CHECK("heads_apply_kernel");
    return KWS_OK;
}

}  // namespace

}  // namespace kws

using namespace kws;

extern "C" {

int kws_heads_apply(const float *emb, int64_t N, int E, const int32_t *rows, const int32_t *key, int64_t key_stride,
                    const int32_t *head_of_key, int64_t K, int64_t R, const float *weights, int64_t weights_count,
                    const int64_t *head_offset, const int32_t *head_classes, int H, int Cmax, float *logits, float *probs,
                    int32_t *pred, void *stream)
{
    if (E < 4 || E > kHbMaxE || E % 4) return fail(KWS_ERR_INVALID, "heads apply: E = %d is not a multiple of 4 in 4 .. %d", E, kHbMaxE);
    if (N < 0 || R < 0) return fail(KWS_ERR_INVALID, "heads apply: N = %lld, R = %lld", (long long)N, (long long)R);
    if (H < 1) return fail(KWS_ERR_INVALID, "heads apply: H = %d heads (at least 1)", H);
    if (Cmax < 2 || Cmax > KWS_HEADS_MAX_CLASSES)
        return fail(KWS_ERR_INVALID, "heads apply: Cmax = %d is outside 2 .. %d (KWS_HEADS_MAX_CLASSES)", Cmax, KWS_HEADS_MAX_CLASSES);
    if (key_stride < 1) return fail(KWS_ERR_INVALID, "heads apply: key_stride = %lld", (long long)key_stride);
    if (weights_count < 0) return fail(KWS_ERR_INVALID, "heads apply: weights_count = %lld", (long long)weights_count);
    if (!emb || !key || !weights || !head_offset || !head_classes) return fail(KWS_ERR_INVALID, "heads apply: null argument");
    if (reinterpret_cast<uintptr_t>(emb) & 15) return fail(KWS_ERR_INVALID, "heads apply: emb must be 16-byte aligned");
    if (head_of_key && K < 1) return fail(KWS_ERR_INVALID, "heads apply: head_of_key with K = %lld keys", (long long)K);
    if (!logits && !probs && !pred) return fail(KWS_ERR_INVALID, "heads apply: logits, probs and pred are all null");
    if (!rows && R > N) return fail(KWS_ERR_INVALID, "heads apply: R = %lld rows of N = %lld without a row array", (long long)R, (long long)N);
    if ((R + kHbRows - 1) / kHbRows > 0x7fffffffll) return fail(KWS_ERR_INVALID, "heads apply: R = %lld rows exceed one launch", (long long)R);
    if (R == 0) return KWS_OK;
    HbShape sh;
    sh.N = N; sh.key_stride = key_stride; sh.K = K; sh.R = R; sh.weights_count = weights_count;
    sh.E = E; sh.H = H; sh.Cmax = Cmax;
    sh.cp_log2 = 1;
    while ((1 << sh.cp_log2) < Cmax && sh.cp_log2 < 6) ++sh.cp_log2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Cmax <= 64) return launch_heads_apply<1>(emb, rows, key, head_of_key, weights, head_offset, head_classes, sh, logits, probs, pred, s);
    if (Cmax <= 128) return launch_heads_apply<2>(emb, rows, key, head_of_key, weights, head_offset, head_classes, sh, logits, probs, pred, s);
    return launch_heads_apply<4>(emb, rows, key, head_of_key, weights, head_offset, head_classes, sh, logits, probs, pred, s);
}

}  // extern "C"
