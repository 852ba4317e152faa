// csrc/kws_quant.h -- the int8 models (include/kws.h: kws_model_calibrate[_lite], kws_model_calibrate_hist, kws_quantize_simple_*,
// kws_qmodel_*): the geometry the quantized CNN forwards are built for, the fragment-major weight layout the kernels read, the device
// helpers, the two calibration kernels (one pair for both CNNs, templated on the network), the host helpers of the quantizers and the
// device-side model with its upload.  What the two CNN forward kernels share beyond this is in kws_quant_fwd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kws_common.h"
#include "kws_model_types.h"

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

// Observers of the calibration forwards (kws_quant.hip CnnCal::forward, kws_quant_lite.hip LiteCal::forward): obs(t, v) gets every value
// v >= 0 of quantized tensor t (|v| for a signed tensor), t a compile-time constant once inlined.  CalMax keeps the thread's running
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

// The two calibration passes of a CNN.  Net (CnnCal in kws_quant.hip, LiteCal in kws_quant_lite.hip) gives the number of quantized
// tensors T, the kernel arguments Args (feat, the weight and BatchNorm pointers, amax), the LDS of one clip's fp32 forward Smem, and
// forward(args, features of one clip, smem, obs): plain fp32 loops over 256 threads that hand every value of a quantized tensor to obs
// and end in cal_dense, WITHOUT a barrier after it (it reads a4 only).  Both passes run this one function, so the histogram pass sees
// exactly the values the max pass reduced.  On the host, Net::args(m, params, state) fills the weight pointers of Args.
template <class Args>
__device__ __forceinline__ float bn_relu6(float y, const Args &a, int l, int c)
{
    const float gm = a.gamma[l][c] / sqrtf(a.mv[l][c] + 1e-3f);
    const float v = (y - a.mm[l][c]) * gm + a.beta[l][c];
    return fminf(fmaxf(v, 0.f), 6.f);
}

// Dense(128) + ReLU6 of a4 [kFlat]: tensor t, the last of both networks
template <class Args, class Obs>
__device__ __forceinline__ void cal_dense(const Args &a, const float *a4, int t, Obs &obs)
{
    for (int o = threadIdx.x; o < kD; o += 256) {
        float s = a.db[o];
#pragma unroll 4
        for (int k = 0; k < kFlat; ++k) s += a4[k] * a.dk[k * kD + o];
        obs(t, fminf(fmaxf(s, 0.f), 6.f));
    }
}

// the max pass: one block per clip, max-reduced into amax [T]
template <class Net>
__global__ __launch_bounds__(256) void cal_max_kernel(typename Net::Args a)
{
    __shared__ typename Net::Smem sm;
    __shared__ int red[Net::T];
    const int tid = threadIdx.x;
    CalMax<Net::T> obs;
    if (tid < Net::T) red[tid] = 0;
    Net::forward(a, a.feat + (long)blockIdx.x * (kH0 * kW0), sm, obs);
    // non-negative floats order like their bit patterns as int (a NaN's pattern would win: the host rejects it)
#pragma unroll
    for (int t = 0; t < Net::T; ++t) atomicMax(&red[t], __float_as_int(obs.mx[t]));
    __syncthreads();
    if (tid < Net::T) atomicMax(reinterpret_cast<int *>(a.amax) + tid, red[tid]);
}

template <class Net>
struct HistArgs {
    typename Net::Args c;
    int B;
    float k[Net::T];                  // 2048 / amax_t, 0 for a tensor that gets no counts
    unsigned long long *hist;
};

// the histogram pass, persistent: block b counts clips b, b + grid, ... into its LDS histograms (8 KB per tensor beside the forward's
// Smem: two blocks per CU for simple_cnn, one for simple_cnn_lite) and adds its nonzero bins to hist once at its end
template <class Net>
__global__ __launch_bounds__(256) void cal_hist_kernel(HistArgs<Net> g)
{
    __shared__ typename Net::Smem sm;
    __shared__ unsigned cnt[Net::T * KWS_QUANT_HIST_BINS];
    for (int i = threadIdx.x; i < Net::T * KWS_QUANT_HIST_BINS; i += 256) cnt[i] = 0u;
    CalHist<Net::T> obs;
    obs.cnt = cnt;
#pragma unroll
    for (int t = 0; t < Net::T; ++t) obs.k[t] = g.k[t];
    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();      // the previous clip's Dense stage has read a4; the counters are cleared
        Net::forward(g.c, g.c.feat + (long)b * (kH0 * kW0), sm, obs);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Net::T * KWS_QUANT_HIST_BINS; i += 256) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(g.hist + i, (unsigned long long)c);
    }
}

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

// The argument checks and the launch of a calibration pass of Net (the caller has checked m); name and what are the launch's labels.
template <class Net>
int cal_max_launch(const char *name, const char *what, const kws_model *m, const float *feat, int B, const float *params,
                   const float *state, float *amax, hipStream_t s)
{
    if (B < 0) return fail(KWS_ERR_INVALID, "batch must be >= 0");
    if (B == 0) return KWS_OK;
    if (!feat || !params || !state || !amax) return fail(KWS_ERR_INVALID, "null argument");
    typename Net::Args a = Net::args(m, params, state);
    a.feat = feat;
    a.amax = amax;
    KWS_LAUNCH(name, cal_max_kernel<Net>, dim3(B), dim3(256), 0, s, a);
    KWS_LAUNCH_CHECK(what);
    return KWS_OK;
}
template <class Net>
int cal_hist_launch(const char *name, const char *what, const kws_model *m, const float *feat, int B, const float *params,
                    const float *state, const float *amax_host, uint64_t *hist, hipStream_t s)
{
    if (B < 0) return fail(KWS_ERR_INVALID, "batch must be >= 0");
    if (B == 0) return KWS_OK;
    if (!feat || !params || !state || !amax_host || !hist) return fail(KWS_ERR_INVALID, "null argument");
    HistArgs<Net> g{};
    int rc = hist_factors(amax_host, Net::T, g.k);
    if (rc) return rc;
    g.c = Net::args(m, params, state);
    g.c.feat = feat;
    g.B = B;
    g.hist = reinterpret_cast<unsigned long long *>(hist);
    KWS_LAUNCH(name, cal_hist_kernel<Net>, dim3(hist_grid(reinterpret_cast<const void *>(cal_hist_kernel<Net>), B)), dim3(256), 0, s, g);
    KWS_LAUNCH_CHECK(what);
    return KWS_OK;
}

// The host quantizers of the two CNNs (kws_quant.hip).  check_cnn_geometry: m is a model of `kind` at the default geometry with at
// most KWS_QUANT_MAX_CLASSES classes (`what` opens the message for another kind).  check_method_amax: KWS_ERR_INVALID for an unknown
// method, a non-finite or negative maximum among the T, or max|x| = 0 of the features (t0).
int check_cnn_geometry(const kws_model *m, int kind, const char *what);
int check_method_amax(int method, const float *amax_host, int T);
// Dense and head of a snapshot Q (kws_qsimple_cnn / kws_qsimple_cnn_lite): codes per output channel, Md / Bd from the scales of a4
// (s_in) and d (s_d), Mh and the fp32 head bias
template <class Q>
void quantize_dense_head(const kws_model *m, const float *params_host, double s_in, double s_d, Q *out)
{
    std::vector<double> sw;
    quantize_weight(params_host + m->o_dk, kFlat, kD, out->dense_w, sw);
    for (int c = 0; c < kD; ++c) {
        out->Md[c] = (float)((s_in * sw[c]) / s_d);
        out->Bd[c] = (float)((double)params_host[m->o_db + c] / s_d);
    }
    quantize_weight(params_host + m->o_hk, kD, m->C, out->head_w, sw);
    for (int c = 0; c < m->C; ++c) {
        out->Mh[c] = (float)(s_d * sw[c]);
        out->head_bias[c] = params_host[m->o_hb + c];
    }
}

// The device image of a quantized model (all three kws_qmodel_create*): put() appends a piece at the next multiple of 256 bytes and
// returns its offset; upload() allocates qm->blob on the current device (noted in qm->device), copies the image and returns the
// blob's base, or nullptr with the error set (KWS_ERR_HIP) and nothing left allocated on the device
struct QBlob {
    std::vector<unsigned char> img;
    size_t put(const void *p, size_t n);
    unsigned char *upload(kws_qmodel *qm) const;
};
}  // namespace q8
}  // namespace kws
