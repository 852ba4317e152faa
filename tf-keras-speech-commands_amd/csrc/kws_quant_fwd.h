// csrc/kws_quant_fwd.h -- what the one-kernel int8 forwards of simple_cnn (kws_quant.hip, qforward_kernel) and simple_cnn_lite
// (kws_quant_lite.hip, lite_qforward_kernel) share: the tile a block owns, the haloed int8 maps both networks have (their pooled
// geometry is the same), the feature prologue and stage 4's pooled epilogue.  The functions are called by all 256 threads of the block
// and take no model kind.  The Dense -> head -> softmax / arg-max tail is the same text in both kernels but stays written out in each:
// as a function it left the registers alone and moved lite_qforward_kernel's instruction order, which measured 0.7 % slower at
// B = 16 384 (inlined locals are promoted in another order than locals of the kernel body).
#pragma once
#include "kws_quant.h"

namespace kws {
namespace q8 {

constexpr int kG = 8;                   // clips per block
constexpr int kThreads = 256;           // four waves
// haloed int8 maps: [clip][H + 2][W + 2][C] (stage 3 is stride 2 with 'same' padding 1 before and 1 after on both axes)
constexpr int kXW = kW0 + 2, kXClip = (kH0 + 2) * kXW;                    // 32 x 22 features: 704 B
constexpr int kA1W = 12, kA1Pix = 17 * kA1W, kA1Clip = kA1Pix * kC1;      // 15 x 10 x 16 -> 3264 B
constexpr int kA2W = 7, kA2Pix = 9 * kA2W, kA2Clip = kA2Pix * kC2;        // 7 x 5 x 32   -> 2016 B
constexpr int kA3W = 5, kA3Pix = 6 * kA3W, kA3Clip = kA3Pix * kC3;        // 4 x 3 x 64   -> 1920 B
constexpr int kT4 = kG * 2 * 4 / 16;    // row tiles of stage 4: (clip, pool window, pixel in window) over the 8 of 12 positions pooling keeps
static_assert(kA1Clip % 16 == 0 && kA2Clip % 16 == 0 && kA3Clip % 16 == 0, "16-byte fragment reads");

// t0: codes of the features of clips b0 .. b0 + kG - 1 into X, halo = 0 (a clip past B is all 0); a1's halo = 0.  No barrier.
__device__ __forceinline__ void fwd_prologue(const float *feat, int B, int b0, float inv_s0, int8_t *X, int8_t *A1)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < kG * kXClip; i += kThreads) {
        const int c = i / kXClip, p = i - c * kXClip, y = p / kXW - 1, x = p % kXW - 1;
        int code = 0;
        if (y >= 0 && y < kH0 && x >= 0 && x < kW0 && b0 + c < B) {
            const float v = feat[(long)(b0 + c) * (kH0 * kW0) + y * kW0 + x];
            code = (int)fminf(fmaxf(rintf(__fmul_rn(v, inv_s0)), -127.f), 127.f);
        }
        X[i] = (int8_t)code;
    }
    for (int i = tid; i < kG * kA1Pix; i += kThreads) {
        const int p = i % kA1Pix, y = p / kA1W, x = p % kA1W;
        if (y == 0 || y > 15 || x == 0 || x > 10) *reinterpret_cast<i32x4 *>(A1 + i * kC1) = i32x4{0, 0, 0, 0};
    }
}

// Stage 4's epilogue of one accumulator tile (row tile t of kT4, lane quarter q, channel ch with its M4 / B4): relu, BN + ReLU6, then
// the 2 x 2 max over the lane's four accumulator registers = one pool window -> a4 [clip][wy][channel].  The loops over the tiles
// stay in the kernels, and q comes from the caller: with either in here qforward_kernel got other registers (46 AGPRs) or another
// instruction order.
__device__ __forceinline__ void fwd_pool4(i32x4 acc, int t, int q, int ch, float M, float Bq, int8_t *A4)
{
    const int p = 4 * t + q, c = p >> 1, wy = p & 1;
    int best = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) best = max(best, requant(max(acc[r], 0), M, Bq));
    A4[c * kFlat + wy * kC4 + ch] = (int8_t)best;
}

}  // namespace q8
}  // namespace kws
