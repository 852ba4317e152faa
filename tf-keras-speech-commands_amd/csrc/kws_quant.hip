// csrc/kws_quant.hip -- int8 post-training quantization of simple_cnn (include/kws.h: kws_model_calibrate, kws_quantize_simple_cnn,
// kws_qmodel_*): the per-clip fp32 forward the calibration kernels of kws_quant.h run, the host quantizer, the host helpers the other
// int8 models share (kws_quant.h) and the int8 forward, features to probabilities in ONE kernel.
//
// The forward (qforward_kernel): a block of 256 threads owns kG = 8 clips for the whole network, every activation an int8 code in LDS,
// stored haloed ([clip][row + 1][col + 1][channel], the halo holding code 0 = the "same" padding), so no tap is ever masked:
//   t0     fp32 features -> codes (the halo written as 0 in the same pass)
//   conv1  vector ALU: one thread per (clip, pool window), the nine taps of a pixel packed into three words, v_dot4_i32_i8 against the
//          channel's packed taps, epilogue, 2 x 2 max on the codes
//   conv2  v_mfma_i32_16x16x64_i8, M = pixels of one clip ordered (pool window, pixel in window): the four accumulator registers of a
//          lane ARE one pool window, so pooling is a max over registers.  A lane quarter is one tap (16 channels = one ds_read_b128 of
//          the haloed pixel); K = 9 taps in three k-steps, the unused three tap slots zero.  The six weight fragments stay in registers
//   conv3  M = (clip, output position), 96 rows; a lane quarter is half a tap (32 channels); wave = 16-column tile
//   conv4  M = (clip, pool window, pixel in window) for the 8 of 12 positions pooling keeps; k-step = tap; wave = two column tiles;
//          max(acc, 0) (the layer's relu) before the epilogue, pooled over registers as conv2
//   Dense, head: M = clips (rows 8..15 of the tile read clips 0..7 again and are dropped); the head's logits stay fp32 in LDS, then
//          softmax and the arg-max per clip
// t0 and the pooled epilogue of a conv4 accumulator tile are the functions of kws_quant_fwd.h, shared with lite_qforward_kernel.
// LDS regions are reused as layers die (kLds = 42 240 B: three blocks per CU).  Weights are read fragment-major from global memory (L2-
// resident, 140 KB in all); the epilogue constants likewise.
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "kws_quant_fwd.h"

namespace kws {
namespace q8 {

// regions: a1 and a3 share [0, 26112); t0, then a2, then a4 / d / logits share the rest
constexpr int kOffA1 = 0, kOffA3 = 0;
constexpr int kOffX = kG * kA1Clip, kOffA2 = kOffX, kOffA4 = kOffX;
constexpr int kOffD = kOffA4 + kG * kFlat, kOffLG = kOffD + kG * kD, kOffMS = kOffLG + 4 * kG * kHead;
constexpr int kLds = kOffA2 + kG * kA2Clip;
static_assert(kG * kA3Clip <= kOffX && kOffMS + 8 * kG <= kLds && kOffX + kG * kXClip <= kLds, "LDS regions");
static_assert(kOffX % 16 == 0, "16-byte fragment reads");

struct QFwdArgs {
    const float *feat;
    int B, C;
    float inv_s0;
    const int32_t *w1;
    const i32x4 *f2, *f3, *f4, *fd, *fh;
    const float *ep;
    float *logits, *probs;
    int32_t *argmax;
};

__global__ __launch_bounds__(kThreads) void qforward_kernel(QFwdArgs g)
{
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *X = lds + kOffX, *A1 = lds + kOffA1, *A2 = lds + kOffA2, *A3 = lds + kOffA3, *A4 = lds + kOffA4, *Dv = lds + kOffD;
    float *LG = reinterpret_cast<float *>(lds + kOffLG), *MS = reinterpret_cast<float *>(lds + kOffMS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, li = lane & 15;
    const int b0 = blockIdx.x * kG;
    const float *ep = g.ep;
    const i32x4 zero4 = {0, 0, 0, 0};

    // ---- t0: codes of the features, halo = 0; a1's halo = 0 ----
    fwd_prologue(g.feat, g.B, b0, g.inv_s0, X, A1);
    __syncthreads();

    // ---- conv1 (vector ALU) + BN + ReLU6 + pool: one thread per (clip, pool window) ----
    for (int t = tid; t < kG * 150; t += kThreads) {
        const int c = t / 150, w = t - c * 150, wy = w / 10, wx = w - wy * 10;
        const int8_t *src = X + c * kXClip + (2 * wy) * kXW + 2 * wx;
        int v[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) v[r][s] = src[r * kXW + s];
        int pk[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int dy = p >> 1, dx = p & 1;
            pk[p][0] = pack4(v[dy][dx], v[dy][dx + 1], v[dy][dx + 2], v[dy + 1][dx]);
            pk[p][1] = pack4(v[dy + 1][dx + 1], v[dy + 1][dx + 2], v[dy + 2][dx], v[dy + 2][dx + 1]);
            pk[p][2] = v[dy + 2][dx + 2] & 255;
        }
        int out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int co = 0; co < kC1; ++co) {
            const int k0 = g.w1[3 * co], k1 = g.w1[3 * co + 1], k2 = g.w1[3 * co + 2];
            const float M = ep[kEpM1 + co], Bq = ep[kEpB1 + co];
            int best = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int acc = __builtin_amdgcn_sdot4(pk[p][0], k0, 0, false);
                acc = __builtin_amdgcn_sdot4(pk[p][1], k1, acc, false);
                acc = __builtin_amdgcn_sdot4(pk[p][2], k2, acc, false);
                best = max(best, requant(acc, M, Bq));
            }
            out[co >> 2] |= best << (8 * (co & 3));
        }
        const i32x4 o = {out[0], out[1], out[2], out[3]};
        *reinterpret_cast<i32x4 *>(A1 + c * kA1Clip + ((wy + 1) * kA1W + wx + 1) * kC1) = o;
    }
    __syncthreads();

    // ---- conv2 on the matrix cores + pool; a2's halo = 0 (t0 is dead) ----
    {
        i32x4 bw[kS2][kN2];
#pragma unroll
        for (int s = 0; s < kS2; ++s)
#pragma unroll
            for (int ct = 0; ct < kN2; ++ct) bw[s][ct] = g.f2[(s * kN2 + ct) * 64 + lane];
        // this lane's A row: pixel (li & 3) of pool window 4 t + (li >> 2); the 36th window (padding) re-reads the 35th
        for (int tile = wave; tile < kG * 9; tile += 4) {
            const int c = tile / 9, t = tile - c * 9;
            const int wr = min(4 * t + (li >> 2), 34), y = 2 * (wr / 5) + ((li >> 1) & 1), x = 2 * (wr % 5) + (li & 1);
            const int8_t *base = A1 + c * kA1Clip;
            i32x4 acc[kN2] = {zero4, zero4};
#pragma unroll
            for (int s = 0; s < kS2; ++s) {
                const int tap = 4 * s + q;
                i32x4 a = zero4;
                if (tap < 9) a = *reinterpret_cast<const i32x4 *>(base + ((y + tap / 3) * kA1W + x + tap % 3) * kC1);
#pragma unroll
                for (int ct = 0; ct < kN2; ++ct) acc[ct] = mfma_i8(a, bw[s][ct], acc[ct]);
            }
            const int w = 4 * t + q;      // output rows 4 q + r = the four pixels of window w
            if (w < 35) {
#pragma unroll
                for (int ct = 0; ct < kN2; ++ct) {
                    const int ch = 16 * ct + li;
                    const float M = ep[kEpM2 + ch], Bq = ep[kEpB2 + ch];
                    int best = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) best = max(best, requant(acc[ct][r], M, Bq));
                    A2[c * kA2Clip + ((w / 5 + 1) * kA2W + w % 5 + 1) * kC2 + ch] = (int8_t)best;
                }
            }
        }
        for (int i = tid; i < kG * kA2Pix; i += kThreads) {
            const int p = i % kA2Pix, y = p / kA2W, x = p % kA2W;
            if (y == 0 || y > 7 || x == 0 || x > 5) {
                *reinterpret_cast<i32x4 *>(A2 + i * kC2) = zero4;
                *reinterpret_cast<i32x4 *>(A2 + i * kC2 + 16) = zero4;
            }
        }
    }
    __syncthreads();

    // ---- conv3 (3 x 3, stride 2): wave = column tile; a3's halo = 0 (a1 is dead) ----
    {
        const int ct = wave;
        i32x4 bw[kS3];
#pragma unroll
        for (int s = 0; s < kS3; ++s) bw[s] = g.f3[(s * kN3 + ct) * 64 + lane];
        const int ch = 16 * ct + li;
        const float M = ep[kEpM3 + ch], Bq = ep[kEpB3 + ch];
        for (int t = 0; t < kG * 12 / 16; ++t) {
            const int m = 16 * t + li, c = m / 12, pos = m - c * 12, oy = pos / 3, ox = pos - oy * 3;
            const int8_t *base = A2 + c * kA2Clip + 16 * (q & 1);
            i32x4 acc = zero4;
#pragma unroll
            for (int s = 0; s < kS3; ++s) {
                const int tap = 2 * s + (q >> 1);
                i32x4 a = zero4;
                if (tap < 9) a = *reinterpret_cast<const i32x4 *>(base + ((2 * oy + tap / 3) * kA2W + 2 * ox + tap % 3) * kC2);
                acc = mfma_i8(a, bw[s], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mo = 16 * t + 4 * q + r, co = mo / 12, po = mo - co * 12;
                A3[co * kA3Clip + ((po / 3 + 1) * kA3W + po % 3 + 1) * kC3 + ch] = (int8_t)requant(acc[r], M, Bq);
            }
        }
        for (int i = tid; i < kG * kA3Pix; i += kThreads) {
            const int p = i % kA3Pix, y = p / kA3W, x = p % kA3W;
            if (y == 0 || y > 4 || x == 0 || x > 3)
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<i32x4 *>(A3 + i * kC3 + 16 * u) = zero4;
        }
    }
    __syncthreads();

    // ---- conv4 + relu + BN + ReLU6 + pool (positions of rows 0..3, columns 0..1): wave = column tiles 2 wave, 2 wave + 1 ----
    {
        i32x4 acc[kT4][2];
#pragma unroll
        for (int t = 0; t < kT4; ++t) acc[t][0] = acc[t][1] = zero4;
        const int8_t *base[kT4];
#pragma unroll
        for (int t = 0; t < kT4; ++t) {
            const int p = 4 * t + (li >> 2), c = p >> 1, wy = p & 1, y = 2 * wy + ((li >> 1) & 1), x = li & 1;
            base[t] = A3 + c * kA3Clip + (y * kA3W + x) * kC3 + 16 * q;
        }
#pragma unroll 3
        for (int s = 0; s < kS4; ++s) {
            const i32x4 w0 = g.f4[(s * kN4 + 2 * wave) * 64 + lane], w1 = g.f4[(s * kN4 + 2 * wave + 1) * 64 + lane];
            const int off = ((s / 3) * kA3W + s % 3) * kC3;
#pragma unroll
            for (int t = 0; t < kT4; ++t) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(base[t] + off);
                acc[t][0] = mfma_i8(a, w0, acc[t][0]);
                acc[t][1] = mfma_i8(a, w1, acc[t][1]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch = 16 * (2 * wave + u) + li;
            const float M = ep[kEpM4 + ch], Bq = ep[kEpB4 + ch];
#pragma unroll
            for (int t = 0; t < kT4; ++t) fwd_pool4(acc[t][u], t, q, ch, M, Bq, A4);
        }
    }
    __syncthreads();

    // ---- Dense(128) + ReLU6: rows = clips, wave = column tiles 2 wave, 2 wave + 1 ----
    {
        i32x4 acc[2] = {zero4, zero4};
#pragma unroll
        for (int s = 0; s < kSd; ++s) {
            const i32x4 a = *reinterpret_cast<const i32x4 *>(A4 + (li & (kG - 1)) * kFlat + 64 * s + 16 * q);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[u] = mfma_i8(a, g.fd[(s * kNd + 2 * wave + u) * 64 + lane], acc[u]);
        }
        if (q < kG / 4)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ch = 16 * (2 * wave + u) + li;
                const float M = ep[kEpMd + ch], Bq = ep[kEpBd + ch];
#pragma unroll
                for (int r = 0; r < 4; ++r) Dv[(4 * q + r) * kD + ch] = (int8_t)requant(acc[u][r], M, Bq);
            }
    }
    __syncthreads();

    // ---- head: logits = (float)acc * Mh + bias, waves 0..2 = column tiles ----
    if (wave < kNh) {
        i32x4 acc = zero4;
#pragma unroll
        for (int s = 0; s < kSh; ++s) {
            const i32x4 a = *reinterpret_cast<const i32x4 *>(Dv + (li & (kG - 1)) * kD + 64 * s + 16 * q);
            acc = mfma_i8(a, g.fh[(s * kNh + wave) * 64 + lane], acc);
        }
        const int col = 16 * wave + li;
        if (q < kG / 4 && col < g.C) {
            const float M = ep[kEpMh + col], hb = ep[kEpHb + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * q + r;
                const float lg = affine(acc[r], M, hb);
                LG[c * kHead + col] = lg;
                if (g.logits && b0 + c < g.B) g.logits[(long)(b0 + c) * g.C + col] = lg;
            }
        }
    }
    __syncthreads();

    // ---- softmax / arg-max per clip (first maximum wins, like np.argmax) ----
    if (tid < kG) {
        const float *x = LG + tid * kHead;
        float mx = x[0];
        int am = 0;
        for (int c = 1; c < g.C; ++c)
            if (x[c] > mx) { mx = x[c]; am = c; }
        float s = 0.f;
        for (int c = 0; c < g.C; ++c) s += expf(x[c] - mx);
        MS[2 * tid] = mx;
        MS[2 * tid + 1] = 1.0f / s;
        if (g.argmax && b0 + tid < g.B) g.argmax[b0 + tid] = am;
    }
    __syncthreads();
    if (g.probs)
        for (int i = tid; i < kG * g.C; i += kThreads) {
            const int c = i / g.C, col = i - c * g.C;
            if (b0 + c < g.B) g.probs[(long)(b0 + c) * g.C + col] = expf(LG[c * kHead + col] - MS[2 * c]) * MS[2 * c + 1];
        }
}

// ---- calibration: the fp32 inference forward of one clip (plain loops), every value of a quantized tensor handed to an observer; the
// network the calibration kernels and launchers of kws_quant.h run for simple_cnn (launch labels qcalibrate_kernel / qhist_kernel) ------
struct CnnCal {
    static constexpr int T = KWS_QUANT_TENSORS;
    struct Args {
        const float *feat;
        const float *k[4], *gamma[4], *beta[4], *mm[4], *mv[4];
        const float *dk, *db;
        float *amax;
    };
    struct Smem {
        float x0[kH0 * kW0], a1[15 * 10 * kC1], a2[7 * 5 * kC2], a3[4 * 3 * kC3], a4[kFlat];
    };
    static Args args(const kws_model *m, const float *params, const float *state)
    {
        Args a{};
        for (int l = 0; l < 4; ++l) {
            a.k[l] = params + m->o_k[l]; a.gamma[l] = params + m->o_g[l]; a.beta[l] = params + m->o_b[l];
            a.mm[l] = state + m->o_mm[l]; a.mv[l] = state + m->o_mv[l];
        }
        a.dk = params + m->o_dk; a.db = params + m->o_db;
        return a;
    }
    template <class Obs>
    static __device__ __forceinline__ void forward(const Args &a, const float *f, Smem &sm, Obs &obs);
};

// obs(t, v): v >= 0 is |x| for t0, the activation itself for t1..t5
template <class Obs>
__device__ __forceinline__ void CnnCal::forward(const Args &a, const float *f, Smem &sm, Obs &obs)
{
    const int tid = threadIdx.x;
    float *x0 = sm.x0, *a1 = sm.a1, *a2 = sm.a2, *a3 = sm.a3, *a4 = sm.a4;
    for (int i = tid; i < kH0 * kW0; i += 256) {
        const float v = f[i];
        x0[i] = v;
        obs(0, fabsf(v));
    }
    __syncthreads();
    // conv1 + pool: 15 x 10 x 16 (pad 1 on every side)
    for (int o = tid; o < 150 * kC1; o += 256) {
        const int w = o / kC1, co = o % kC1, wy = w / 10, wx = w % 10;
        float best = 0.f;
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = 2 * wx + (p & 1);
            float s = 0.f;
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int iy = y + ky - 1, ix = x + kx - 1;
                    if (iy >= 0 && iy < kH0 && ix >= 0 && ix < kW0) s += x0[iy * kW0 + ix] * a.k[0][(ky * 3 + kx) * kC1 + co];
                }
            best = fmaxf(best, bn_relu6(s, a, 0, co));
        }
        a1[o] = best;
        obs(1, best);
    }
    __syncthreads();
    // conv2 + pool: 7 x 5 x 32 of the 15 x 10 map (pad 1)
    for (int o = tid; o < 35 * kC2; o += 256) {
        const int w = o / kC2, co = o % kC2, wy = w / 5, wx = w % 5;
        float best = 0.f;
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = 2 * wx + (p & 1);
            float s = 0.f;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                if (iy < 0 || iy >= 15 || ix < 0 || ix >= 10) continue;
#pragma unroll 4
                for (int ci = 0; ci < kC1; ++ci) s += a1[(iy * 10 + ix) * kC1 + ci] * a.k[1][(tap * kC1 + ci) * kC2 + co];
            }
            best = fmaxf(best, bn_relu6(s, a, 1, co));
        }
        a2[o] = best;
        obs(2, best);
    }
    __syncthreads();
    // conv3: stride 2, 'same' (pad 1 before): 4 x 3 x 64
    for (int o = tid; o < 12 * kC3; o += 256) {
        const int pos = o / kC3, co = o % kC3, oy = pos / 3, ox = pos % 3;
        float s = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = 2 * oy + tap / 3 - 1, ix = 2 * ox + tap % 3 - 1;
            if (iy < 0 || iy >= 7 || ix < 0 || ix >= 5) continue;
#pragma unroll 4
            for (int ci = 0; ci < kC2; ++ci) s += a2[(iy * 5 + ix) * kC2 + ci] * a.k[2][(tap * kC2 + ci) * kC3 + co];
        }
        const float v = bn_relu6(s, a, 2, co);
        a3[o] = v;
        obs(3, v);
    }
    __syncthreads();
    // conv4 (relu) + BN + ReLU6 + pool: 2 x 1 x 128 of the 4 x 3 map
    for (int o = tid; o < kFlat; o += 256) {
        const int wy = o / kC4, co = o % kC4;
        float best = 0.f;
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = p & 1;
            float s = 0.f;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                if (iy < 0 || iy >= 4 || ix < 0 || ix >= 3) continue;
#pragma unroll 4
                for (int ci = 0; ci < kC3; ++ci) s += a3[(iy * 3 + ix) * kC3 + ci] * a.k[3][(tap * kC3 + ci) * kC4 + co];
            }
            best = fmaxf(best, bn_relu6(fmaxf(s, 0.f), a, 3, co));
        }
        a4[o] = best;
        obs(4, best);
    }
    __syncthreads();
    cal_dense(a, a4, 5, obs);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_cnn_geometry(const kws_model *m, int kind, const char *what)
{
    if (!m) return fail(KWS_ERR_INVALID, "null model");
    if (m->kind != kind) return fail(KWS_ERR_UNSUPPORTED, "%s only (model kind %d)", what, m->kind);
    if (m->n_features != kH0 || m->feature_size != kW0)
        return fail(KWS_ERR_UNSUPPORTED, "int8 quantization covers the default %dx%d geometry, not %dx%d", kH0, kW0, m->n_features, m->feature_size);
    if (m->C > KWS_QUANT_MAX_CLASSES) return fail(KWS_ERR_UNSUPPORTED, "int8 quantization covers up to %d classes, not %d", KWS_QUANT_MAX_CLASSES, m->C);
    return KWS_OK;
}
int check_model(const kws_model *m) { return check_cnn_geometry(m, KWS_SIMPLE_CNN, "int8 quantization covers simple_cnn"); }

int check_method_amax(int method, const float *amax_host, int T)
{
    if (method != KWS_QUANT_MAX && method != KWS_QUANT_RELU6 && method != KWS_QUANT_KL)
        return fail(KWS_ERR_INVALID, "unknown quantization method %d", method);
    for (int t = 0; t < T; ++t) {
        const double v = amax_host[t];
        if (!std::isfinite(v) || v < 0.0) return fail(KWS_ERR_INVALID, "calibrated maximum of t%d is %g (must be finite and >= 0)", t, v);
    }
    if (amax_host[0] == 0.f) return fail(KWS_ERR_INVALID, "calibrated max|x| of the features is 0");
    return KWS_OK;
}

// per-output-channel MAX_ABS of W (K x N, row-major): q and s_wc
void quantize_weight(const float *W, int K, int N, int8_t *q, std::vector<double> &sw)
{
    sw.assign(N, 1.0);
    for (int c = 0; c < N; ++c) {
        double r = 0.0;
        for (int k = 0; k < K; ++k) r = std::max(r, std::fabs((double)W[(size_t)k * N + c]));
        sw[c] = r == 0.0 ? 1.0 : r / 127.0;
        for (int k = 0; k < K; ++k) {
            const double v = std::rint((double)W[(size_t)k * N + c] / sw[c]);
            q[(size_t)k * N + c] = (int8_t)std::min(127.0, std::max(-127.0, v));
        }
    }
}

// the fragment-major image of an int8 K x N matrix (kws_quant.h)
void pack_frags(const int8_t *W, int K, int N, int S, int NCT, std::vector<int8_t> &out)
{
    out.assign((size_t)S * NCT * 64 * 16, 0);
    for (int s = 0; s < S; ++s)
        for (int ct = 0; ct < NCT; ++ct)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j) {
                    const int k = 64 * s + 16 * (l >> 4) + j, col = 16 * ct + (l & 15);
                    if (k < K && col < N) out[(((size_t)s * NCT + ct) * 64 + l) * 16 + j] = W[(size_t)k * N + col];
                }
}

size_t QBlob::put(const void *p, size_t n)
{
    const size_t off = al256(img.size());
    img.resize(off + n);
    std::memcpy(img.data() + off, p, n);
    return off;
}

unsigned char *QBlob::upload(kws_qmodel *qm) const
{
    if (hipGetDevice(&qm->device) != hipSuccess || hipMalloc(&qm->blob, img.size()) != hipSuccess) {
        (void)hipGetLastError();
        qm->blob = nullptr;
        fail(KWS_ERR_HIP, "no HIP device / out of device memory for the quantized model");
        return nullptr;
    }
    if (hipMemcpy(qm->blob, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(qm->blob);
        qm->blob = nullptr;
        fail(KWS_ERR_HIP, "upload of the quantized model failed");
        return nullptr;
    }
    return static_cast<unsigned char *>(qm->blob);
}

int hist_grid(const void *kernel, int B)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, 0) != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = 1; }
    return std::min(B, nb * device_cus());
}

// 2048 / amax_t per tensor (0 for amax_t == 0: no counts); KWS_ERR_INVALID for a non-finite or negative maximum
int hist_factors(const float *amax_host, int T, float *k)
{
    for (int t = 0; t < T; ++t) {
        const double v = amax_host[t];
        if (!std::isfinite(v) || v < 0.0) return fail(KWS_ERR_INVALID, "calibrated maximum of t%d is %g (must be finite and >= 0)", t, v);
        k[t] = v > 0.0 ? (float)(2048.0 / v) : 0.f;
    }
    return KWS_OK;
}

// the KL search of include/kws.h over one histogram -> i* (0 for an empty one)
int kl_best_bin(const uint64_t *h)
{
    constexpr int kBins = KWS_QUANT_HIST_BINS, kGroups = 128;
    // prefix sums of the counts and of the nonzero bins: every partial sum is an integer, exact in uint64 (and in double below 2^53)
    std::vector<uint64_t> pre(kBins + 1, 0), nz(kBins + 1, 0);
    for (int j = 0; j < kBins; ++j) {
        pre[j + 1] = pre[j] + h[j];
        nz[j + 1] = nz[j] + (h[j] != 0);
    }
    if (pre[kBins] == 0) return 0;
    std::vector<double> Q(kBins);
    double best = INFINITY;
    int best_i = kBins;
    for (int i = kGroups; i <= kBins; ++i) {
        const double tail = (double)(pre[kBins] - pre[i]);
        if (tail > 0.0 && h[i - 1] == 0) continue;             // p_{i-1} > 0, q_{i-1} = 0: KL_i = +inf
        double sumQ = 0.0;
        for (int g = 0; g < kGroups; ++g) {
            const int j0 = g * i / kGroups, j1 = (g + 1) * i / kGroups;
            const uint64_t n = nz[j1] - nz[j0];
            const double v = n ? (double)(pre[j1] - pre[j0]) / (double)n : 0.0;
            for (int j = j0; j < j1; ++j) {
                Q[j] = h[j] ? v : 0.0;
                sumQ += Q[j];
            }
        }
        if (sumQ == 0.0) continue;
        const double sumP = (double)pre[kBins];                 // sum P = N
        double kl = 0.0;
        for (int j = 0; j < i; ++j) {
            const double P = (double)h[j] + (j == i - 1 ? tail : 0.0);
            if (P == 0.0) continue;
            const double p = P / sumP, q = Q[j] / sumQ;
            kl += p * std::log(p / q);
        }
        if (kl < best) { best = kl; best_i = i; }
    }
    return best_i;
}

}  // namespace q8
}  // namespace kws

using namespace kws;
using namespace kws::q8;

extern "C" {

int kws_model_calibrate(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                        float *amax, void *stream)
{
    (void)ws; (void)ws_bytes;
    int rc = check_model(m);
    if (rc) return rc;
    return cal_max_launch<CnnCal>("qcalibrate_kernel", "calibration", m, feat, B, params, state, amax, static_cast<hipStream_t>(stream));
}

int kws_model_calibrate_hist(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                             const float *amax_host, uint64_t *hist, void *stream)
{
    (void)ws; (void)ws_bytes;
    if (m && m->kind == KWS_SIMPLE_CNN_LITE)
        return lite_calibrate_hist(m, feat, B, params, state, amax_host, hist, static_cast<hipStream_t>(stream));
    int rc = check_model(m);
    if (rc) return rc;
    return cal_hist_launch<CnnCal>("qhist_kernel", "calibration histograms", m, feat, B, params, state, amax_host, hist,
                                   static_cast<hipStream_t>(stream));
}

int kws_quant_kl_ranges(const uint64_t *hist_host, const float *amax_host, int T, float *ranges_out, int32_t *bins_out)
{
    if (T < 0) return fail(KWS_ERR_INVALID, "tensor count must be >= 0");
    if (T > 0 && (!hist_host || !amax_host || !ranges_out)) return fail(KWS_ERR_INVALID, "null argument");
    for (int t = 0; t < T; ++t)
        if (!std::isfinite(amax_host[t]) || amax_host[t] < 0.f)
            return fail(KWS_ERR_INVALID, "calibrated maximum of t%d is %g (must be finite and >= 0)", t, (double)amax_host[t]);
    // one host thread per tensor (about 2 M log terms each; the searches are independent)
    std::vector<int> best(T, 0);
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) {
        try {
            pool.emplace_back([&best, hist_host, t] { best[t] = kl_best_bin(hist_host + (size_t)t * KWS_QUANT_HIST_BINS); });
        } catch (...) {       // no thread to be had: search here
            best[t] = kl_best_bin(hist_host + (size_t)t * KWS_QUANT_HIST_BINS);
        }
    }
    if (T > 0) best[0] = kl_best_bin(hist_host);
    for (auto &th : pool) th.join();
    for (int t = 0; t < T; ++t) {
        ranges_out[t] = (float)((double)best[t] * (double)amax_host[t] / (double)KWS_QUANT_HIST_BINS);
        if (bins_out) bins_out[t] = best[t];
    }
    return KWS_OK;
}

int kws_quantize_simple_cnn(const kws_model *m, const float *params_host, const float *state_host, const float *amax_host, int method,
                            kws_qsimple_cnn *out)
{
    int rc = check_model(m);
    if (rc) return rc;
    if (!params_host || !state_host || !amax_host || !out) return fail(KWS_ERR_INVALID, "null argument");
    rc = check_method_amax(method, amax_host, KWS_QUANT_TENSORS);
    if (rc) return rc;
    double A[KWS_QUANT_TENSORS];
    for (int t = 0; t < KWS_QUANT_TENSORS; ++t) {
        const double v = amax_host[t];
        A[t] = t == 0 ? v : method == KWS_QUANT_RELU6 || v == 0.0 ? 6.0 : std::min(v, 6.0);
    }
    std::memset(out, 0, sizeof(*out));
    out->num_classes = m->C;
    out->method = method;
    double s[KWS_QUANT_TENSORS];
    for (int t = 0; t < KWS_QUANT_TENSORS; ++t) {
        s[t] = A[t] / 127.0;
        out->amax[t] = A[t];
        out->scale[t] = s[t];
    }
    out->inv_s0 = (float)(1.0 / s[0]);
    const int ci[4] = {1, kC1, kC2, kC3}, co[4] = {kC1, kC2, kC3, kC4};
    int8_t *qw[4] = {out->conv_w1, out->conv_w2, out->conv_w3, out->conv_w4};
    float *Mo[4] = {out->M1, out->M2, out->M3, out->M4}, *Bo[4] = {out->B1, out->B2, out->B3, out->B4};
    std::vector<double> sw;
    const double eps = (double)1e-3f;      // kBnEps widened
    for (int l = 0; l < 4; ++l) {
        quantize_weight(params_host + m->o_k[l], 9 * ci[l], co[l], qw[l], sw);
        for (int c = 0; c < co[l]; ++c) {
            const double g = (double)params_host[m->o_g[l] + c] / std::sqrt((double)state_host[m->o_mv[l] + c] + eps);
            const double h = (double)params_host[m->o_b[l] + c] - (double)state_host[m->o_mm[l] + c] * g;
            Mo[l][c] = (float)(((s[l] * sw[c]) * g) / s[l + 1]);
            Bo[l][c] = (float)(h / s[l + 1]);
        }
    }
    quantize_dense_head(m, params_host, s[4], s[5], out);
    return KWS_OK;
}

int kws_qmodel_create(const kws_model *m, const kws_qsimple_cnn *q, kws_qmodel **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = check_model(m);
    if (rc) return rc;
    if (!q) return fail(KWS_ERR_INVALID, "null argument");
    if (q->num_classes != m->C) return fail(KWS_ERR_INVALID, "quantized model has %d classes, the model %d", q->num_classes, m->C);
    if (!std::isfinite(q->inv_s0) || !(q->inv_s0 > 0.f)) return fail(KWS_ERR_INVALID, "inv_s0 must be finite and > 0");
    const float *ep = q->M1;
    for (int i = 0; i < kEpCount; ++i)
        if (!std::isfinite(ep[i])) return fail(KWS_ERR_INVALID, "epilogue constant %d is not finite", i);
    // conv1: per channel the nine taps packed four to a word (byte j of word w = tap 4 w + j)
    std::vector<int32_t> w1(3 * kC1, 0);
    for (int c = 0; c < kC1; ++c)
        for (int tap = 0; tap < 9; ++tap)
            w1[3 * c + tap / 4] |= (int32_t)((uint32_t)(uint8_t)q->conv_w1[tap * kC1 + c] << (8 * (tap % 4)));
    std::vector<int8_t> f2, f3, f4, fd, fh;
    pack_frags(q->conv_w2, 9 * kC1, kC2, kS2, kN2, f2);
    pack_frags(q->conv_w3, 9 * kC2, kC3, kS3, kN3, f3);
    pack_frags(q->conv_w4, 9 * kC3, kC4, kS4, kN4, f4);
    pack_frags(q->dense_w, kFlat, kD, kSd, kNd, fd);
    pack_frags(q->head_w, kD, m->C, kSh, kNh, fh);
    QBlob img;
    const size_t o1 = img.put(w1.data(), w1.size() * 4), o2 = img.put(f2.data(), f2.size()), o3 = img.put(f3.data(), f3.size()),
                 o4 = img.put(f4.data(), f4.size()), od = img.put(fd.data(), fd.size()), oh = img.put(fh.data(), fh.size()),
                 oe = img.put(ep, sizeof(float) * kEpCount);
    auto *qm = new kws_qmodel();
    qm->kind = KWS_SIMPLE_CNN;
    qm->C = m->C;
    qm->inv_s0 = q->inv_s0;
    const unsigned char *b = img.upload(qm);
    if (!b) { delete qm; return KWS_ERR_HIP; }
    qm->w1 = reinterpret_cast<const int32_t *>(b + o1);
    qm->f2 = reinterpret_cast<const i32x4 *>(b + o2);
    qm->f3 = reinterpret_cast<const i32x4 *>(b + o3);
    qm->f4 = reinterpret_cast<const i32x4 *>(b + o4);
    qm->fd = reinterpret_cast<const i32x4 *>(b + od);
    qm->fh = reinterpret_cast<const i32x4 *>(b + oh);
    qm->ep = reinterpret_cast<const float *>(b + oe);
    *out = qm;
    return KWS_OK;
}

void kws_qmodel_destroy(kws_qmodel *q)
{
    if (!q) return;
    if (q->blob) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != q->device) (void)hipSetDevice(q->device);
        (void)hipFree(q->blob);
        if (cur != q->device && cur >= 0) (void)hipSetDevice(cur);
    }
    delete q;
}

int64_t kws_qmodel_workspace_bytes(const kws_qmodel *q, int B)
{
    (void)q; (void)B;
    return 0;
}

int kws_qmodel_forward(const kws_qmodel *q, const float *feat, int B, void *ws, size_t ws_bytes, float *logits, float *probs,
                       int32_t *argmax, void *stream)
{
    (void)ws; (void)ws_bytes;
    if (!q) return fail(KWS_ERR_INVALID, "null quantized model");
    if (B < 0) return fail(KWS_ERR_INVALID, "batch must be >= 0");
    if (B == 0) return KWS_OK;
    if (!feat) return fail(KWS_ERR_INVALID, "null features");
    if (q->kind == KWS_SIMPLE_CNN_LITE) return lite_qforward(q, feat, B, logits, probs, argmax, static_cast<hipStream_t>(stream));
    if (q->kind == KWS_SIMPLE_GRU || q->kind == KWS_SIMPLE_LSTM)
        return rnn_qforward(q, feat, B, logits, probs, argmax, static_cast<hipStream_t>(stream));
    int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(qforward_kernel), kLds);
    if (rc) return rc;
    QFwdArgs a{feat, B, q->C, q->inv_s0, q->w1, q->f2, q->f3, q->f4, q->fd, q->fh, q->ep, logits, probs, argmax};
    KWS_LAUNCH("qforward_kernel", qforward_kernel, dim3(blocks_for(B, kG)), dim3(kThreads), kLds, static_cast<hipStream_t>(stream), a);
    KWS_LAUNCH_CHECK("int8 forward");
    return KWS_OK;
}

}  // extern "C"
