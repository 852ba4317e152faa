// csrc/kws_quant_lite.hip -- int8 post-training quantization of simple_cnn_lite (include/kws.h: kws_model_calibrate_lite,
// kws_quantize_simple_cnn_lite, kws_qmodel_create_lite; kws_qmodel_forward dispatches here): the per-clip fp32 forward the calibration
// kernels of kws_quant.h run, the host quantizer and the int8 forward, features to probabilities in ONE kernel.
//
// The forward (lite_qforward_kernel) follows qforward_kernel (kws_quant.hip): a block of 256 threads owns kG = 8 clips for the whole
// network, every activation an int8 code in LDS, the maps a 3 x 3 stage reads stored haloed ([clip][row + 1][col + 1][channel], halo
// = code 0 = the "same" padding), so no tap is ever masked:
//   t0       fp32 features -> codes (halo written as 0 in the same pass)
//   stage 1  vector ALU, one thread per (clip, pool window): the nine taps of each of the window's four pixels packed into three
//            words, v_dot4_i32_i8 against the packed depthwise taps -> u1; pointwise 1 (K = 1) as one integer multiply-add per channel,
//            epilogue, 2 x 2 max on the codes
//   dw 2-4   vector ALU, one thread per (clip, pixel, 4-channel word): nine words of the haloed input, byte-unpacked multiply-adds
//            against the channel word's nine tap words -> four u codes, stored as rows of the next pointwise GEMM; only the pixels
//            pooling keeps are computed (14 x 10 of 15 x 10 for stage 2, 4 x 2 of 4 x 3 for stage 4)
//   pw 2-4   one k-step of v_mfma_i32_16x16x64_i8 per row tile (K = 16, 32 zero-padded to 64 on both sides), the int32 bias as the
//            accumulator's initial value.  M is ordered (clip, pool window, pixel in window) for the pooled stages, so the four
//            accumulator registers of a lane are one pool window and pooling is a max over registers (stage 2 as conv2, stage 4 as
//            conv4 of the simple_cnn kernel); stage 3 rows are (clip, output position)
//   Dense, head, softmax, arg-max: those of qforward_kernel
//   t0 and the pooled epilogue of a stage-4 accumulator tile are the functions of kws_quant_fwd.h both kernels call
// LDS: two regions reused as stages die: R0 = a1 -> a2 -> a3 -> a4 / d / logits, R1 = t0 -> u2 -> u3 -> u4 (kLLds = 44 544 B, three
// blocks per CU).  Weights and constants are packed by kws_qmodel_create_lite and read from global memory (L2-resident, 56 KB).
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "kws_quant_fwd.h"

namespace kws {
namespace q8 {
namespace {

// the depthwise outputs, rows of the pointwise GEMMs (the haloed a_l maps are those of kws_quant_fwd.h)
constexpr int kU2Rows = 36 * 4, kU2Clip = kU2Rows * kC1;                  // (window 0..35, pixel 0..3) x 16: 2304 B (window 35 unused)
constexpr int kU3Clip = 12 * kC2;                                         // 4 x 3 positions x 32: 384 B
constexpr int kU4Clip = 8 * kC3;                                          // (window 0..1, pixel 0..3) x 64: 512 B
constexpr int kR1 = kG * kA1Clip;                                         // R0 = [0, kR1), R1 = [kR1, kLLds)
constexpr int kOffA1 = 0, kOffA2 = 0, kOffA3 = 0, kOffA4 = 0, kOffD = kG * kFlat, kOffLG = kOffD + kG * kD, kOffMS = kOffLG + 4 * kG * kHead;
constexpr int kOffX = kR1, kOffU2 = kR1, kOffU3 = kR1, kOffU4 = kR1;
constexpr int kLLds = kR1 + kG * kU2Clip;
static_assert(kG * kA2Clip <= kR1 && kG * kA3Clip <= kR1 && kOffMS + 8 * kG <= kR1, "R0");
static_assert(kG * kXClip <= kG * kU2Clip && kG * kU3Clip <= kG * kU2Clip && kG * kU4Clip <= kG * kU2Clip, "R1");
static_assert(kR1 % 16 == 0, "16-byte reads");

// u = clamp(rint((float)dacc * Mu), -127, 127)
__device__ __forceinline__ int requant_u(int acc, float Mu)
{
    const float r = rintf((float)acc * Mu);
    return (int)fminf(fmaxf(r, -127.f), 127.f);
}
__device__ __forceinline__ int sbyte(int w, int j) { return (int)(int8_t)(w >> (8 * j)); }

// one thread's depthwise word: four channels of one output pixel over the nine taps of a haloed map (row stride `rs` bytes, pixel
// stride `ps` bytes), packed back into a word of four u codes
__device__ __forceinline__ int dw_word(const int8_t *src, int rs, int ps, const int32_t *wt, const float *Mu)
{
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int a = *reinterpret_cast<const int *>(src + (tap / 3) * rs + (tap % 3) * ps), w = wt[tap];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += sbyte(a, j) * sbyte(w, j);
    }
    return pack4(requant_u(acc[0], Mu[0]), requant_u(acc[1], Mu[1]), requant_u(acc[2], Mu[2]), requant_u(acc[3], Mu[3]));
}

struct LQFwdArgs {
    const float *feat;
    int B, C;
    float inv_s0;
    const int32_t *dw1, *dw2, *dw3, *dw4;
    const int8_t *pw1;
    const i32x4 *f2, *f3, *f4, *fd, *fh;
    const float *ep;
    const int32_t *bq;
    float *logits, *probs;
    int32_t *argmax;
};

__global__ __launch_bounds__(kThreads) void lite_qforward_kernel(LQFwdArgs g)
{
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *X = lds + kOffX, *A1 = lds + kOffA1, *U2 = lds + kOffU2, *A2 = lds + kOffA2, *U3 = lds + kOffU3, *A3 = lds + kOffA3;
    int8_t *U4 = lds + kOffU4, *A4 = lds + kOffA4, *Dv = lds + kOffD;
    float *LG = reinterpret_cast<float *>(lds + kOffLG), *MS = reinterpret_cast<float *>(lds + kOffMS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, li = lane & 15;
    const int b0 = blockIdx.x * kG;
    const float *ep = g.ep;
    const int32_t *bq = g.bq;
    const i32x4 zero4 = {0, 0, 0, 0};

    // ---- t0: codes of the features, halo = 0; a1's halo = 0 ----
    fwd_prologue(g.feat, g.B, b0, g.inv_s0, X, A1);
    __syncthreads();

    // ---- stage 1: depthwise (one channel) + pointwise (K = 1) + bias + BN + ReLU6 + pool, one thread per (clip, pool window) ----
    {
        const int k0 = g.dw1[0], k1 = g.dw1[1], k2 = g.dw1[2];
        const float Mu = ep[kLEpMu1];
        for (int t = tid; t < kG * 150; t += kThreads) {
            const int c = t / 150, w = t - c * 150, wy = w / 10, wx = w - wy * 10;
            const int8_t *src = X + c * kXClip + (2 * wy) * kXW + 2 * wx;
            int v[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) v[r][s] = src[r * kXW + s];
            int u[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int dy = p >> 1, dx = p & 1;
                int acc = __builtin_amdgcn_sdot4(pack4(v[dy][dx], v[dy][dx + 1], v[dy][dx + 2], v[dy + 1][dx]), k0, 0, false);
                acc = __builtin_amdgcn_sdot4(pack4(v[dy + 1][dx + 1], v[dy + 1][dx + 2], v[dy + 2][dx], v[dy + 2][dx + 1]), k1, acc, false);
                acc = __builtin_amdgcn_sdot4(v[dy + 2][dx + 2] & 255, k2, acc, false);
                u[p] = requant_u(acc, Mu);
            }
            int out[4] = {0, 0, 0, 0};
#pragma unroll
            for (int co = 0; co < kC1; ++co) {
                const int wq = g.pw1[co], b = bq[kLBq1 + co];
                const float M = ep[kLEpM1 + co], Bq = ep[kLEpB1 + co];
                int best = 0;
#pragma unroll
                for (int p = 0; p < 4; ++p) best = max(best, requant(u[p] * wq + b, M, Bq));
                out[co >> 2] |= best << (8 * (co & 3));
            }
            const i32x4 o = {out[0], out[1], out[2], out[3]};
            *reinterpret_cast<i32x4 *>(A1 + c * kA1Clip + ((wy + 1) * kA1W + wx + 1) * kC1) = o;
        }
    }
    __syncthreads();

    // ---- depthwise 2 (t0 is dead): the 14 x 10 pixels pooling keeps, rows (window, pixel in window) of u2 ----
    for (int t = tid; t < kG * 140 * 4; t += kThreads) {
        const int c = t / 560, r = t - c * 560, px = r >> 2, wd = r & 3, y = px / 10, x = px - y * 10;
        const int row = 4 * ((y >> 1) * 5 + (x >> 1)) + 2 * (y & 1) + (x & 1);
        *reinterpret_cast<int *>(U2 + c * kU2Clip + row * kC1 + 4 * wd) =
            dw_word(A1 + c * kA1Clip + (y * kA1W + x) * kC1 + 4 * wd, kA1W * kC1, kC1, g.dw2 + 9 * wd, ep + kLEpMu2 + 4 * wd);
    }
    __syncthreads();

    // ---- pointwise 2 on the matrix cores (K = 16 in lane quarter 0) + bias + BN + ReLU6 + pool; a2's halo = 0 (a1 is dead) ----
    {
        i32x4 bw[2];
        int b[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            bw[ct] = g.f2[ct * 64 + lane];
            b[ct] = bq[kLBq2 + 16 * ct + li];
        }
        for (int tile = wave; tile < kG * 9; tile += 4) {
            const int c = tile / 9, t = tile - c * 9;
            const int m = min(16 * t + li, 139);          // the 36th window (padding) re-reads the 35th's last pixel
            i32x4 a = zero4;
            if (q == 0) a = *reinterpret_cast<const i32x4 *>(U2 + c * kU2Clip + m * kC1);
            i32x4 acc[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const i32x4 bias = {b[ct], b[ct], b[ct], b[ct]};
                acc[ct] = mfma_i8(a, bw[ct], bias);
            }
            const int w = 4 * t + q;      // output rows 4 q + r = the four pixels of window w
            if (w < 35) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int ch = 16 * ct + li;
                    const float M = ep[kLEpM2 + ch], Bq = ep[kLEpB2 + ch];
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

    // ---- depthwise 3 (stride 2, padding 1 / 1): 4 x 3 positions x 8 words (u2 is dead) ----
    for (int t = tid; t < kG * 12 * 8; t += kThreads) {
        const int c = t / 96, r = t - c * 96, pos = r >> 3, wd = r & 7, oy = pos / 3, ox = pos - oy * 3;
        *reinterpret_cast<int *>(U3 + c * kU3Clip + pos * kC2 + 4 * wd) =
            dw_word(A2 + c * kA2Clip + (2 * oy * kA2W + 2 * ox) * kC2 + 4 * wd, kA2W * kC2, kC2, g.dw3 + 9 * wd, ep + kLEpMu3 + 4 * wd);
    }
    __syncthreads();

    // ---- pointwise 3 (K = 32 in lane quarters 0, 1) + bias + relu + BN + ReLU6: wave = column tile; a3's halo = 0 (a2 is dead) ----
    {
        const int ct = wave, ch = 16 * ct + li;
        const i32x4 bw = g.f3[ct * 64 + lane];
        const int b = bq[kLBq3 + ch];
        const i32x4 bias = {b, b, b, b};
        const float M = ep[kLEpM3 + ch], Bq = ep[kLEpB3 + ch];
        for (int t = 0; t < kG * 12 / 16; ++t) {
            i32x4 a = zero4;
            if (q < 2) a = *reinterpret_cast<const i32x4 *>(U3 + (16 * t + li) * kC2 + 16 * q);
            const i32x4 acc = mfma_i8(a, bw, bias);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mo = 16 * t + 4 * q + r, co = mo / 12, po = mo - co * 12;
                A3[co * kA3Clip + ((po / 3 + 1) * kA3W + po % 3 + 1) * kC3 + ch] = (int8_t)requant(max(acc[r], 0), M, Bq);
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

    // ---- depthwise 4: the 4 x 2 positions pooling keeps, rows (window, pixel in window) x 16 words (u3 is dead) ----
    for (int t = tid; t < kG * 8 * 16; t += kThreads) {
        const int c = t >> 7, r = t & 127, pos = r >> 4, wd = r & 15, y = 2 * (pos >> 2) + ((pos >> 1) & 1), x = pos & 1;
        *reinterpret_cast<int *>(U4 + c * kU4Clip + pos * kC3 + 4 * wd) =
            dw_word(A3 + c * kA3Clip + (y * kA3W + x) * kC3 + 4 * wd, kA3W * kC3, kC3, g.dw4 + 9 * wd, ep + kLEpMu4 + 4 * wd);
    }
    __syncthreads();

    // ---- pointwise 4 (K = 64) + bias + relu + BN + ReLU6 + pool: wave = column tiles 2 wave, 2 wave + 1 (a3 is dead) ----
    {
        i32x4 bw[2], bias[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bw[u] = g.f4[(2 * wave + u) * 64 + lane];
            const int b = bq[kLBq4 + 16 * (2 * wave + u) + li];
            bias[u] = i32x4{b, b, b, b};
        }
        i32x4 acc[kT4][2];
#pragma unroll
        for (int t = 0; t < kT4; ++t) {
            const i32x4 a = *reinterpret_cast<const i32x4 *>(U4 + (16 * t + li) * kC3 + 16 * q);
            acc[t][0] = mfma_i8(a, bw[0], bias[0]);
            acc[t][1] = mfma_i8(a, bw[1], bias[1]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch = 16 * (2 * wave + u) + li;
            const float M = ep[kLEpM4 + ch], Bq = ep[kLEpB4 + ch];
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
                const float M = ep[kLEpMd + ch], Bq = ep[kLEpBd + ch];
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
            const float M = ep[kLEpMh + col], hb = ep[kLEpHb + col];
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

// ---- calibration: the fp32 inference forward of one clip (plain loops), the network the calibration kernels and launchers of
// kws_quant.h run for simple_cnn_lite (launch labels lite_qcalibrate_kernel / lite_qhist_kernel) --------------------------------------

// depthwise 3 x 3 output (oy, ox, channel c) of an H x W x C map, 'same' padding 1 before (stride 1 or 2)
__device__ float ldw(const float *in, int H, int W, int C, const float *k, int oy, int ox, int c, int stride)
{
    float s = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = stride * oy + tap / 3 - 1, ix = stride * ox + tap % 3 - 1;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += in[(iy * W + ix) * C + c] * k[tap * C + c];
    }
    return s;
}
// pointwise output channel co of one pixel: bias + sum over ci, optionally relu
__device__ float lpw(const float *u, int CI, const float *k, const float *b, int CO, int co, bool relu)
{
    float s = 0.f;
#pragma unroll 4
    for (int ci = 0; ci < CI; ++ci) s += u[ci] * k[ci * CO + co];
    s += b[co];
    return relu ? fmaxf(s, 0.f) : s;
}

struct LiteCal {
    static constexpr int T = KWS_QLITE_TENSORS;
    struct Args {
        const float *feat;
        const float *dwk[4], *pwk[4], *pwb[4], *gamma[4], *beta[4], *mm[4], *mv[4];
        const float *dk, *db;
        float *amax;
    };
    struct Smem {
        float x0[kH0 * kW0], u1[kH0 * kW0], a1[150 * kC1], u2[150 * kC1], a2[35 * kC2], u3[12 * kC2], a3[12 * kC3], u4[12 * kC3], a4[kFlat];
    };
    static Args args(const kws_model *m, const float *params, const float *state)
    {
        Args a{};
        for (int l = 0; l < 4; ++l) {
            a.dwk[l] = params + m->o_dwk[l]; a.pwk[l] = params + m->o_pwk[l]; a.pwb[l] = params + m->o_pwb[l];
            a.gamma[l] = params + m->o_g[l]; a.beta[l] = params + m->o_b[l];
            a.mm[l] = state + m->o_mm[l]; a.mv[l] = state + m->o_mv[l];
        }
        a.dk = params + m->o_dk; a.db = params + m->o_db;
        return a;
    }
    template <class Obs>
    static __device__ __forceinline__ void forward(const Args &a, const float *f, Smem &sm, Obs &obs);
};

// obs(t, v) as in kws_quant.h (|u_l| for the signed depthwise outputs)
template <class Obs>
__device__ __forceinline__ void LiteCal::forward(const Args &a, const float *f, Smem &sm, Obs &obs)
{
    const int tid = threadIdx.x;
    float *x0 = sm.x0, *u1 = sm.u1, *a1 = sm.a1, *u2 = sm.u2, *a2 = sm.a2, *u3 = sm.u3, *a3 = sm.a3, *u4 = sm.u4, *a4 = sm.a4;
    for (int i = tid; i < kH0 * kW0; i += 256) {
        const float v = f[i];
        x0[i] = v;
        obs(0, fabsf(v));
    }
    __syncthreads();
    for (int o = tid; o < kH0 * kW0; o += 256) {
        u1[o] = ldw(x0, kH0, kW0, 1, a.dwk[0], o / kW0, o % kW0, 0, 1);
        obs(1, fabsf(u1[o]));
    }
    __syncthreads();
    for (int o = tid; o < 150 * kC1; o += 256) {      // pointwise 1 + BN + ReLU6 + pool: 15 x 10 x 16
        const int w = o / kC1, co = o % kC1, wy = w / 10, wx = w % 10;
        float best = 0.f;
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = 2 * wx + (p & 1);
            best = fmaxf(best, bn_relu6(lpw(u1 + y * kW0 + x, 1, a.pwk[0], a.pwb[0], kC1, co, false), a, 0, co));
        }
        a1[o] = best;
        obs(2, best);
    }
    __syncthreads();
    for (int o = tid; o < 150 * kC1; o += 256) {
        u2[o] = ldw(a1, 15, 10, kC1, a.dwk[1], (o / kC1) / 10, (o / kC1) % 10, o % kC1, 1);
        obs(3, fabsf(u2[o]));
    }
    __syncthreads();
    for (int o = tid; o < 35 * kC2; o += 256) {       // pointwise 2 + BN + ReLU6 + pool: 7 x 5 x 32
        const int w = o / kC2, co = o % kC2, wy = w / 5, wx = w % 5;
        float best = 0.f;
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = 2 * wx + (p & 1);
            best = fmaxf(best, bn_relu6(lpw(u2 + (y * 10 + x) * kC1, kC1, a.pwk[1], a.pwb[1], kC2, co, false), a, 1, co));
        }
        a2[o] = best;
        obs(4, best);
    }
    __syncthreads();
    for (int o = tid; o < 12 * kC2; o += 256) {       // depthwise 3, stride 2: 4 x 3 x 32
        u3[o] = ldw(a2, 7, 5, kC2, a.dwk[2], (o / kC2) / 3, (o / kC2) % 3, o % kC2, 2);
        obs(5, fabsf(u3[o]));
    }
    __syncthreads();
    for (int o = tid; o < 12 * kC3; o += 256) {
        const float v = bn_relu6(lpw(u3 + (o / kC3) * kC2, kC2, a.pwk[2], a.pwb[2], kC3, o % kC3, true), a, 2, o % kC3);
        a3[o] = v;
        obs(6, v);
    }
    __syncthreads();
    for (int o = tid; o < 12 * kC3; o += 256) {
        u4[o] = ldw(a3, 4, 3, kC3, a.dwk[3], (o / kC3) / 3, (o / kC3) % 3, o % kC3, 1);
        obs(7, fabsf(u4[o]));
    }
    __syncthreads();
    for (int o = tid; o < kFlat; o += 256) {          // pointwise 4 + relu + BN + ReLU6 + pool: 2 x 1 x 128
        const int wy = o / kC4, co = o % kC4;
        float best = 0.f;
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * wy + (p >> 1), x = p & 1;
            best = fmaxf(best, bn_relu6(lpw(u4 + (y * 3 + x) * kC3, kC3, a.pwk[3], a.pwb[3], kC4, co, true), a, 3, co));
        }
        a4[o] = best;
        obs(8, best);
    }
    __syncthreads();
    cal_dense(a, a4, 9, obs);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_lite(const kws_model *m) { return check_cnn_geometry(m, KWS_SIMPLE_CNN_LITE, "the lite int8 entry points cover simple_cnn_lite"); }

constexpr int kCin[4] = {1, kC1, kC2, kC3}, kCout[4] = {kC1, kC2, kC3, kC4};

static_assert(offsetof(kws_qsimple_cnn_lite, head_bias) - offsetof(kws_qsimple_cnn_lite, Mu1) == sizeof(float) * kLEpHb &&
                  sizeof(kws_qsimple_cnn_lite::head_bias) == sizeof(float) * (kLEpCount - kLEpHb),
              "the epilogue constants of kws_qsimple_cnn_lite are one array in the order of kLEp*");
static_assert(offsetof(kws_qsimple_cnn_lite, bq4) - offsetof(kws_qsimple_cnn_lite, bq1) == sizeof(int32_t) * kLBq4 &&
                  sizeof(kws_qsimple_cnn_lite::bq4) == sizeof(int32_t) * (kLBqCount - kLBq4),
              "the pointwise biases of kws_qsimple_cnn_lite are one array in the order of kLBq*");

}  // namespace

int lite_qforward(const kws_qmodel *q, const float *feat, int B, float *logits, float *probs, int32_t *argmax, hipStream_t s)
{
    int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(lite_qforward_kernel), kLLds);
    if (rc) return rc;
    LQFwdArgs a{feat, B, q->C, q->inv_s0, q->dw[0], q->dw[1], q->dw[2], q->dw[3], q->pw1,
                q->fp[1], q->fp[2], q->fp[3], q->fd, q->fh, q->ep, q->bq, logits, probs, argmax};
    KWS_LAUNCH("lite_qforward_kernel", lite_qforward_kernel, dim3(blocks_for(B, kG)), dim3(kThreads), kLLds, s, a);
    KWS_LAUNCH_CHECK("int8 lite forward");
    return KWS_OK;
}

int lite_calibrate_hist(const kws_model *m, const float *feat, int B, const float *params, const float *state, const float *amax_host,
                        uint64_t *hist, hipStream_t s)
{
    int rc = check_lite(m);
    if (rc) return rc;
    return cal_hist_launch<LiteCal>("lite_qhist_kernel", "lite calibration histograms", m, feat, B, params, state, amax_host, hist, s);
}

}  // namespace q8
}  // namespace kws

using namespace kws;
using namespace kws::q8;

extern "C" {

int kws_model_calibrate_lite(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                             float *amax, void *stream)
{
    (void)ws; (void)ws_bytes;
    int rc = check_lite(m);
    if (rc) return rc;
    return cal_max_launch<LiteCal>("lite_qcalibrate_kernel", "lite calibration", m, feat, B, params, state, amax,
                                   static_cast<hipStream_t>(stream));
}

int kws_quantize_simple_cnn_lite(const kws_model *m, const float *params_host, const float *state_host, const float *amax_host, int method,
                                 kws_qsimple_cnn_lite *out)
{
    int rc = check_lite(m);
    if (rc) return rc;
    if (!params_host || !state_host || !amax_host || !out) return fail(KWS_ERR_INVALID, "null argument");
    rc = check_method_amax(method, amax_host, KWS_QLITE_TENSORS);
    if (rc) return rc;
    double A[KWS_QLITE_TENSORS];
    for (int t = 0; t < KWS_QLITE_TENSORS; ++t) {
        const double v = amax_host[t];
        const bool relu6_tensor = t == 9 || (t > 0 && t % 2 == 0);     // a1..a4, d; the odd t are the depthwise outputs u1..u4
        if (t == 0) A[t] = v;
        else if (relu6_tensor) A[t] = method == KWS_QUANT_RELU6 || v == 0.0 ? 6.0 : std::min(v, 6.0);
        else A[t] = v == 0.0 ? 1.0 : v;
    }
    std::memset(out, 0, sizeof(*out));
    out->num_classes = m->C;
    out->method = method;
    double s[KWS_QLITE_TENSORS];
    for (int t = 0; t < KWS_QLITE_TENSORS; ++t) {
        s[t] = A[t] / 127.0;
        out->amax[t] = A[t];
        out->scale[t] = s[t];
    }
    out->inv_s0 = (float)(1.0 / s[0]);
    int8_t *qdw[4] = {out->dw_w1, out->dw_w2, out->dw_w3, out->dw_w4}, *qpw[4] = {out->pw_w1, out->pw_w2, out->pw_w3, out->pw_w4};
    int32_t *bqo[4] = {out->bq1, out->bq2, out->bq3, out->bq4};
    float *Mu[4] = {out->Mu1, out->Mu2, out->Mu3, out->Mu4};
    float *Mo[4] = {out->M1, out->M2, out->M3, out->M4}, *Bo[4] = {out->B1, out->B2, out->B3, out->B4};
    std::vector<double> swd, swp;
    const double eps = (double)1e-3f;      // kBnEps widened
    const double bq_max = 8388608.0;       // 2^23
    for (int l = 0; l < 4; ++l) {
        const double s_in = s[2 * l], s_u = s[2 * l + 1], s_out = s[2 * l + 2];
        quantize_weight(params_host + m->o_dwk[l], 9, kCin[l], qdw[l], swd);
        for (int c = 0; c < kCin[l]; ++c) Mu[l][c] = (float)((s_in * swd[c]) / s_u);
        quantize_weight(params_host + m->o_pwk[l], kCin[l], kCout[l], qpw[l], swp);
        for (int c = 0; c < kCout[l]; ++c) {
            const double b = std::rint((double)params_host[m->o_pwb[l] + c] / (s_u * swp[c]));
            bqo[l][c] = (int32_t)std::max(-bq_max, std::min(bq_max, b));
            const double g = (double)params_host[m->o_g[l] + c] / std::sqrt((double)state_host[m->o_mv[l] + c] + eps);
            const double h = (double)params_host[m->o_b[l] + c] - (double)state_host[m->o_mm[l] + c] * g;
            Mo[l][c] = (float)(((s_u * swp[c]) * g) / s_out);
            Bo[l][c] = (float)(h / s_out);
        }
    }
    quantize_dense_head(m, params_host, s[8], s[9], out);
    return KWS_OK;
}

int kws_qmodel_create_lite(const kws_model *m, const kws_qsimple_cnn_lite *q, kws_qmodel **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = check_lite(m);
    if (rc) return rc;
    if (!q) return fail(KWS_ERR_INVALID, "null argument");
    if (q->num_classes != m->C) return fail(KWS_ERR_INVALID, "quantized model has %d classes, the model %d", q->num_classes, m->C);
    if (!std::isfinite(q->inv_s0) || !(q->inv_s0 > 0.f)) return fail(KWS_ERR_INVALID, "inv_s0 must be finite and > 0");
    const float *ep = q->Mu1;
    for (int i = 0; i < kLEpCount; ++i)
        if (!std::isfinite(ep[i])) return fail(KWS_ERR_INVALID, "epilogue constant %d is not finite", i);
    // depthwise 1: the nine taps of the one channel packed four to a word (byte j of word w = tap 4 w + j); stages 2..4: per 4-channel
    // word wd the nine tap words, byte j of word [wd][tap] = qdw[tap][4 wd + j]
    std::vector<int32_t> dw1(3, 0);
    for (int tap = 0; tap < 9; ++tap) dw1[tap / 4] |= (int32_t)((uint32_t)(uint8_t)q->dw_w1[tap] << (8 * (tap % 4)));
    const int8_t *qdw[3] = {q->dw_w2, q->dw_w3, q->dw_w4};
    std::vector<int32_t> dwn[3];
    for (int l = 0; l < 3; ++l) {
        const int C = kCin[l + 1];
        dwn[l].assign(9 * C / 4, 0);
        for (int wd = 0; wd < C / 4; ++wd)
            for (int tap = 0; tap < 9; ++tap)
                for (int j = 0; j < 4; ++j)
                    dwn[l][9 * wd + tap] |= (int32_t)((uint32_t)(uint8_t)qdw[l][tap * C + 4 * wd + j] << (8 * j));
    }
    std::vector<int8_t> f2, f3, f4, fd, fh;
    pack_frags(q->pw_w2, kC1, kC2, 1, kC2 / 16, f2);
    pack_frags(q->pw_w3, kC2, kC3, 1, kC3 / 16, f3);
    pack_frags(q->pw_w4, kC3, kC4, 1, kC4 / 16, f4);
    pack_frags(q->dense_w, kFlat, kD, kSd, kNd, fd);
    pack_frags(q->head_w, kD, m->C, kSh, kNh, fh);
    QBlob img;
    const size_t o1 = img.put(dw1.data(), dw1.size() * 4), o2 = img.put(dwn[0].data(), dwn[0].size() * 4),
                 o3 = img.put(dwn[1].data(), dwn[1].size() * 4), o4 = img.put(dwn[2].data(), dwn[2].size() * 4), op = img.put(q->pw_w1, kC1),
                 of2 = img.put(f2.data(), f2.size()), of3 = img.put(f3.data(), f3.size()), of4 = img.put(f4.data(), f4.size()),
                 od = img.put(fd.data(), fd.size()), oh = img.put(fh.data(), fh.size()), oe = img.put(ep, sizeof(float) * kLEpCount),
                 ob = img.put(q->bq1, sizeof(int32_t) * kLBqCount);
    auto *qm = new kws_qmodel();
    qm->kind = KWS_SIMPLE_CNN_LITE;
    qm->C = m->C;
    qm->inv_s0 = q->inv_s0;
    const unsigned char *b = img.upload(qm);
    if (!b) { delete qm; return KWS_ERR_HIP; }
    qm->dw[0] = reinterpret_cast<const int32_t *>(b + o1);
    qm->dw[1] = reinterpret_cast<const int32_t *>(b + o2);
    qm->dw[2] = reinterpret_cast<const int32_t *>(b + o3);
    qm->dw[3] = reinterpret_cast<const int32_t *>(b + o4);
    qm->pw1 = reinterpret_cast<const int8_t *>(b + op);
    qm->fp[1] = reinterpret_cast<const i32x4 *>(b + of2);
    qm->fp[2] = reinterpret_cast<const i32x4 *>(b + of3);
    qm->fp[3] = reinterpret_cast<const i32x4 *>(b + of4);
    qm->fd = reinterpret_cast<const i32x4 *>(b + od);
    qm->fh = reinterpret_cast<const i32x4 *>(b + oh);
    qm->ep = reinterpret_cast<const float *>(b + oe);
    qm->bq = reinterpret_cast<const int32_t *>(b + ob);
    *out = qm;
    return KWS_OK;
}

}  // extern "C"
