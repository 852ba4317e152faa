// csrc/kws_quant.h -- int8 simple_cnn and simple_cnn_lite (include/kws.h: kws_model_calibrate[_lite], kws_quantize_simple_cnn[_lite],
// kws_qmodel_*): the geometry the quantized forwards are built for, the fragment-major weight layout their kernels read, the helpers
// both share and the device-side model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kws.h"

namespace kws {
namespace q8 {
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The default geometry: 30 x 20 -> conv1 + pool 15 x 10 x 16 -> conv2 + pool 7 x 5 x 32 -> conv3 (stride 2) 4 x 3 x 64 -> conv4 + pool
// 2 x 1 x 128 -> Dense 128 -> head C.
constexpr int kH0 = 30, kW0 = 20;
constexpr int kC1 = 16, kC2 = 32, kC3 = 64, kC4 = 128, kFlat = 256, kD = 128;
constexpr int kHead = KWS_QUANT_MAX_CLASSES;   // head columns padded to three 16-column tiles

// Fragment-major weights of the matrix layers (v_mfma_i32_16x16x64_i8).  Fragment (s, ct) of a layer with K reduced rows (HWIO
// flattening k = tap * CI + ci) and N columns is 64 lanes x 16 bytes: byte j of lane l = W[k = 64 s + 16 (l >> 4) + j][16 ct + (l & 15)],
// 0 past K or N; stored at ((s * NCT + ct) * 64 + l).  For conv2 (CI = 16) a lane quarter is one tap, for conv3 (CI = 32) half a tap,
// for conv4 (CI = 64) a k-step is one tap: the A side reads the same 16 channels of one haloed input pixel.
constexpr int kS2 = 3, kN2 = 2;     // K = 144 (9 taps x 16, padded to 192)
constexpr int kS3 = 5, kN3 = 4;     // K = 288 (padded to 320)
constexpr int kS4 = 9, kN4 = 8;     // K = 576
constexpr int kSd = 4, kNd = 8;     // K = 256
constexpr int kSh = 2, kNh = 3;     // K = 128, C <= 48
// epilogue constants, one fp32 array: M1 B1 M2 B2 M3 B3 M4 B4 Md Bd Mh head_bias (the order of kws_qsimple_cnn)
constexpr int kEpM1 = 0, kEpB1 = 16, kEpM2 = 32, kEpB2 = 64, kEpM3 = 96, kEpB3 = 160, kEpM4 = 224, kEpB4 = 352;
constexpr int kEpMd = 480, kEpBd = 608, kEpMh = 736, kEpHb = 784, kEpCount = 832;

__device__ __forceinline__ i32x4 mfma_i8(i32x4 a, i32x4 b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }

// (float)acc * M + B with the multiply and the add rounded separately: HIP compiles with fp-contract=fast and __fmul_rn / __fadd_rn are
// plain operators, so without the pragma the pair becomes one v_fma_f32 (one rounding) and the logits move by an ulp
__device__ __forceinline__ float affine(int acc, float M, float B)
{
#pragma clang fp contract(off)
    return (float)acc * M + B;
}
// code = clamp(rint((float)acc * M + Bq), 0, 127)
__device__ __forceinline__ int requant(int acc, float M, float Bq)
{
    const float r = rintf(affine(acc, M, Bq));
    return (int)fminf(fmaxf(r, 0.f), 127.f);
}

__device__ __forceinline__ int pack4(int a, int b, int c, int d) { return (a & 255) | (b & 255) << 8 | (c & 255) << 16 | (int)((unsigned)d << 24); }

// Observers of the calibration forwards (kws_quant.hip cal_forward, kws_quant_lite.hip lite_cal_forward): obs(t, v) gets every value v
// >= 0 of quantized tensor t (|v| for a signed tensor), t a compile-time constant once inlined.  CalMax keeps the thread's running
// maxima; CalHist counts v != 0 into the block's LDS histograms [T][KWS_QUANT_HIST_BINS]: bin = min((int)(v * k_t), 2047), k_t = 2048
// / amax_t (0: tensor t is not counted) -- one fp32 multiply, nothing to contract.
template <int T>
struct CalMax {
    float mx[T];
    __device__ __forceinline__ CalMax()
    {
#pragma unroll
        for (int t = 0; t < T; ++t) mx[t] = 0.f;
    }
    __device__ __forceinline__ void operator()(int t, float v) { mx[t] = fmaxf(mx[t], v); }
};
template <int T>
struct CalHist {
    unsigned *cnt;
    float k[T];
    __device__ __forceinline__ void operator()(int t, float v)
    {
        if (v != 0.f && k[t] > 0.f) atomicAdd(cnt + t * KWS_QUANT_HIST_BINS + min((int)__fmul_rn(v, k[t]), KWS_QUANT_HIST_BINS - 1), 1u);
    }
};

// host helpers (kws_quant.hip): per-output-channel MAX_ABS of a K x N row-major matrix; the fragment-major image of an int8 K x N matrix
void quantize_weight(const float *W, int K, int N, int8_t *q, std::vector<double> &sw);
void pack_frags(const int8_t *W, int K, int N, int S, int NCT, std::vector<int8_t> &out);

// simple_cnn_lite (kws_quant_lite.hip).  Stages: depthwise 3 x 3 (vector ALU) -> u_l codes; pointwise as one k-step of
// v_mfma_i32_16x16x64_i8 (K = 16 and 32 zero-padded to 64; pointwise 1, K = 1, on the vector ALU).  Epilogue constants, one fp32 array
// in the order of kws_qsimple_cnn_lite: Mu1..Mu4, M1 B1 .. M4 B4, Md Bd Mh head_bias; the int32 pointwise biases bq1..bq4 in another.
constexpr int kLEpMu1 = 0, kLEpMu2 = 1, kLEpMu3 = 17, kLEpMu4 = 49, kLEpM1 = 113, kLEpB1 = 129, kLEpM2 = 145, kLEpB2 = 177;
constexpr int kLEpM3 = 209, kLEpB3 = 273, kLEpM4 = 337, kLEpB4 = 465, kLEpMd = 593, kLEpBd = 721, kLEpMh = 849, kLEpHb = 897;
constexpr int kLEpCount = 945;
constexpr int kLBq1 = 0, kLBq2 = 16, kLBq3 = 48, kLBq4 = 112, kLBqCount = 240;
}  // namespace q8
}  // namespace kws

struct kws_qmodel {
    int kind = KWS_SIMPLE_CNN;            // KWS_SIMPLE_CNN or KWS_SIMPLE_CNN_LITE: which forward kws_qmodel_forward runs
    int C = 0;
    int device = -1;
    float inv_s0 = 0.f;
    void *blob = nullptr;                 // one device allocation holding everything below
    const int32_t *w1 = nullptr;          // conv1: [16][3] int32 = the 9 taps of a channel packed 4 per word (tap 8 alone in the third)
    const kws::q8::i32x4 *f2 = nullptr, *f3 = nullptr, *f4 = nullptr, *fd = nullptr, *fh = nullptr;
    const float *ep = nullptr;            // kEpCount floats (simple_cnn) / kLEpCount (simple_cnn_lite)
    // simple_cnn_lite: depthwise taps [stage][channel word][tap] as int32 words of 4 channels (stage 1: the 9 taps of its one channel
    // packed 4 per word, as conv1 above), pointwise 1 [16] int8 in one array, fragments of pointwise 2..4, the int32 biases
    const int32_t *dw[4] = {nullptr, nullptr, nullptr, nullptr};
    const int8_t *pw1 = nullptr;
    const kws::q8::i32x4 *fp[4] = {nullptr, nullptr, nullptr, nullptr};
    const int32_t *bq = nullptr;          // kLBqCount
    // simple_gru / simple_lstm (kws_quant_rnn.hip): T steps of F features; fragments of kernel and recurrent_kernel (fh: the head, ep:
    // the column scales and biases)
    int T = 0, F = 0;
    const kws::q8::i32x4 *rw = nullptr, *ru = nullptr;
};

namespace kws {
namespace q8 {
int lite_qforward(const kws_qmodel *q, const float *feat, int B, float *logits, float *probs, int32_t *argmax, hipStream_t s);
// the dynamic-range int8 simple_gru / simple_lstm forward (kws_quant_rnn.hip)
int rnn_qforward(const kws_qmodel *q, const float *feat, int B, float *logits, float *probs, int32_t *argmax, hipStream_t s);
// kws_model_calibrate_hist for simple_cnn_lite (kws_quant_lite.hip)
int lite_calibrate_hist(const kws_model *m, const float *feat, int B, const float *params, const float *state, const float *amax_host,
                        uint64_t *hist, hipStream_t s);
// kws_quant.hip: the grid of a persistent calibration-histogram kernel, min(B, resident blocks of the device); the bin factors k_t =
// (float)(2048.0 / amax_t), 0 where amax_t == 0 (KWS_ERR_INVALID for a non-finite or negative maximum)
int hist_grid(const void *kernel, int B);
int hist_factors(const float *amax_host, int T, float *k);
}  // namespace q8
}  // namespace kws
