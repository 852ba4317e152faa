// csrc/kws_quant_rnn.hip -- int8 dynamic-range quantization of simple_gru and simple_lstm (include/kws.h: kws_quantize_simple_rnn,
// kws_qmodel_create_rnn; kws_qmodel_forward dispatches here): the host quantizer and the forward, features to probabilities in ONE
// kernel.
//
// The forward (qrnn_kernel<G>, G = 3 gates for the GRU, 4 for the LSTM): ONE wave owns 16 clips (the M of v_mfma_i32_16x16x64_i8)
// for the whole sequence, so the recurrence is wave-local and crosses no block barrier.
//   - The W and U codes of all 3 G column tiles are B fragments in registers for the whole sequence (K = F and 48, each zero-padded to
//     one k-step of 64): 4 VGPRs per tile and matrix.
//   - Step t: x_t is quantized in the A layout (lane (q, li) holds clip li, bytes k = 16 q + j), its row maximum reduced over the four
//     lane quarters; then 3 G independent MFMAs for x_t W and 3 G for h_{t-1} U.  x_t is loaded one step ahead.
//   - The C layout puts (clip 4 q + r, column 16 ct + li) in lane (q, li), register r: the 3 G tiles of one unit group are the G gates
//     of the same (clip, unit), so the gate arithmetic is lane-local; h (and the LSTM's c) stay fp32 registers.
//   - h' is requantized: max|h| over the lane's three unit tiles, then over the 16 lanes of its quarter (xor shuffles: max is exact and
//     order-free); the codes go from the C layout to the A layout through a 1 KB LDS tile, ping-ponged by step.  The workgroup is one
//     wave, so its barrier is a wave barrier.
//   - Head: one MFMA per 16-class tile on the codes of h_T; logits to LDS, then the softmax / arg-max of the other int8 heads.
// Computing every step's input product before the recurrence (one MFMA per (step, tile) up front) would keep T x 16 x N fp32
// pre-activations: 276 KB for the GRU at T = 30, more than a CU's LDS.  The x_t W products do not depend on h, so they sit at the head
// of each step's MFMA batch instead.
#include <cmath>
#include <cstring>
#include <vector>

#include "kws_common.h"
#include "kws_gru.h"
#include "kws_model_types.h"
#include "kws_quant.h"

namespace kws {
namespace q8 {

constexpr int kRU = KWS_QRNN_UNITS;               // 48 hidden units
constexpr int kRN = 4 * kRU;                      // widest gate row (LSTM), the stride of the epilogue arrays
// epilogue constants, one fp32 array: sW[kRN] sU[kRN] b0[kRN] b1[kRN] (LSTM: b in b0, b1 unused) sH[48] head_bias[48]
constexpr int kQsW = 0, kQsU = kRN, kQb0 = 2 * kRN, kQb1 = 3 * kRN, kQsH = 4 * kRN, kQhb = kQsH + KWS_QUANT_MAX_CLASSES;
constexpr int kQEpCount = kQhb + KWS_QUANT_MAX_CLASSES;

struct QRnnArgs {
    const float *feat;
    int B, T, F, C;
    const i32x4 *fw, *fu, *fh;          // fragments of kernel, recurrent_kernel (3 G tiles each) and the head (3 tiles)
    const float *ep;
    float *logits, *probs;
    int32_t *argmax;
};

// fp32 row quantization of include/kws.h: code = clamp(rint(v * inv), -127, 127), inv = 127 / m (IEEE division), 0 for m == 0
__device__ __forceinline__ int qcode(float v, float inv, bool live)
{
    return live ? (int)fminf(fmaxf(rintf(v * inv), -127.f), 127.f) : 0;
}

template <int G>
__global__ __launch_bounds__(64) void qrnn_kernel(QRnnArgs g)
{
#pragma clang fp contract(off)
    constexpr int NT = 3 * G;                         // 16-column tiles of the gate rows
    __shared__ __attribute__((aligned(16))) int8_t hq[2][16][64];
    __shared__ float LG[16][KWS_QUANT_MAX_CLASSES];
    __shared__ float MS[16][2];
    const int lane = threadIdx.x, q = lane >> 4, li = lane & 15;
    const int b0 = blockIdx.x * 16;
    const i32x4 zero4 = {0, 0, 0, 0};
    const float *ep = g.ep;

    i32x4 W[NT], U[NT];
    float sW[NT], sU[NT], bx[NT], bh[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        W[ct] = g.fw[ct * 64 + lane];
        U[ct] = g.fu[ct * 64 + lane];
        const int col = 16 * ct + li;
        sW[ct] = ep[kQsW + col];
        sU[ct] = ep[kQsU + col];
        bx[ct] = ep[kQb0 + col];
        bh[ct] = ep[kQb1 + col];
    }

    // this lane's clip in the A layout (li) and its features: F values per step, quarter q holding k = 16 q .. 16 q + 15
    const int T = g.T, F = g.F;
    const bool inb = b0 + li < g.B;
    const float *xrow = g.feat + (long)(inb ? b0 + li : 0) * T * F;
    float xn[16];
    auto load_x = [&](int t) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = 16 * q + j;
            xn[j] = inb && k < F ? xrow[t * F + k] : 0.f;
        }
    };
    load_x(0);

    float h[3][4], c[3][4], sh[4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[j][r] = c[j][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) sh[r] = 0.f;
    i32x4 ah = zero4;                                 // codes of h_0 = 0 (scale 0)
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        float xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = xn[j];
        if (t + 1 < T) load_x(t + 1);

        // ---- x_t: row max over the clip's F values (16 per quarter, then across the quarters), codes in the A layout ----
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) mx = fmaxf(mx, fabsf(xv[j]));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const bool xl = mx > 0.f;
        const float xinv = xl ? 127.f / mx : 0.f;
        int xw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w)
            xw[w] = pack4(qcode(xv[4 * w], xinv, xl), qcode(xv[4 * w + 1], xinv, xl), qcode(xv[4 * w + 2], xinv, xl),
                          qcode(xv[4 * w + 3], xinv, xl));
        const i32x4 ax = {xw[0], xw[1], xw[2], xw[3]};
        const float sxa = mx / 127.f;                 // the scale of clip li
        float sx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) sx[r] = __shfl(sxa, 4 * q + r, 64);     // of clip 4 q + r: lane 4 q + r holds it

        // ---- 3 G independent MFMAs for x_t W, then 3 G for h_{t-1} U ----
        i32x4 accx[NT], acch[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) accx[ct] = mfma_i8(ax, W[ct], zero4);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acch[ct] = mfma_i8(ah, U[ct], zero4);

        // ---- gates (lane-local): unit group j = tiles j, 3 + j, 6 + j (, 9 + j) ----
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float X[G], H[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const int ct = 3 * k + j;
                    X[k] = ((float)accx[ct][r] * sx[r]) * sW[ct];
                    H[k] = ((float)acch[ct][r] * sh[r]) * sU[ct];
                }
                if constexpr (G == 3) {
                    const float mxz = X[0] + bx[j], mhz = H[0] + bh[j];
                    const float mxr = X[1] + bx[3 + j], mhr = H[1] + bh[3 + j];
                    const float mxh = X[2] + bx[6 + j], mhh = H[2] + bh[6 + j];
                    const float z = sigmoidf_(mxz + mhz), rg = sigmoidf_(mxr + mhr);
                    const float hh = mxh + rg * mhh;
                    h[j][r] = z * h[j][r] + (1.f - z) * hh;
                } else {
                    const float ig = sigmoidf_((X[0] + H[0]) + bx[j]), fg = sigmoidf_((X[1] + H[1]) + bx[3 + j]);
                    const float gg = tanh_fast_((X[2] + H[2]) + bx[6 + j]), og = sigmoidf_((X[3] + H[3]) + bx[9 + j]);
                    c[j][r] = fg * c[j][r] + ig * gg;
                    h[j][r] = og * tanh_fast_(c[j][r]);
                }
            }

        // ---- requantize h' (row = clip 4 q + r over the lane's 3 tiles and the quarter's 16 lanes) -> LDS -> A layout ----
        int8_t(*hw)[64] = hq[cur];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = fmaxf(fmaxf(fabsf(h[0][r]), fabsf(h[1][r])), fabsf(h[2][r]));
            m = fmaxf(m, __shfl_xor(m, 1, 64));
            m = fmaxf(m, __shfl_xor(m, 2, 64));
            m = fmaxf(m, __shfl_xor(m, 4, 64));
            m = fmaxf(m, __shfl_xor(m, 8, 64));
            const bool hl = m > 0.f;
            const float hinv = hl ? 127.f / m : 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) hw[4 * q + r][16 * j + li] = (int8_t)qcode(h[j][r], hinv, hl);
            sh[r] = m / 127.f;
        }
        __syncthreads();
        ah = q < 3 ? *reinterpret_cast<const i32x4 *>(&hq[cur][li][16 * q]) : zero4;
        cur ^= 1;
    }

    // ---- head on the codes of h_T: logit = ((float)acc * s_hT) * s_c + bias_c ----
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) {
        const i32x4 acc = mfma_i8(ah, g.fh[ct * 64 + lane], zero4);
        const int col = 16 * ct + li;
        if (col < g.C) {
            const float M = ep[kQsH + col], hb = ep[kQhb + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = 4 * q + r;
                const float lg = ((float)acc[r] * sh[r]) * M + hb;
                LG[cl][col] = lg;
                if (g.logits && b0 + cl < g.B) g.logits[(long)(b0 + cl) * g.C + col] = lg;
            }
        }
    }
    __syncthreads();

    // ---- softmax / arg-max per clip (first maximum wins), as qforward_kernel ----
    if (lane < 16) {
        const float *x = LG[lane];
        float mxl = x[0];
        int am = 0;
        for (int k = 1; k < g.C; ++k)
            if (x[k] > mxl) { mxl = x[k]; am = k; }
        float s = 0.f;
        for (int k = 0; k < g.C; ++k) s += expf(x[k] - mxl);
        MS[lane][0] = mxl;
        MS[lane][1] = 1.0f / s;
        if (g.argmax && b0 + lane < g.B) g.argmax[b0 + lane] = am;
    }
    __syncthreads();
    if (g.probs)
        for (int i = lane; i < 16 * g.C; i += 64) {
            const int cl = i / g.C, col = i - cl * g.C;
            if (b0 + cl < g.B) g.probs[(long)(b0 + cl) * g.C + col] = expf(LG[cl][col] - MS[cl][0]) * MS[cl][1];
        }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_rnn(const kws_model *m)
{
    if (!m) return fail(KWS_ERR_INVALID, "null model");
    if (m->kind != KWS_SIMPLE_GRU && m->kind != KWS_SIMPLE_LSTM)
        return fail(KWS_ERR_UNSUPPORTED, "dynamic-range int8 quantization covers simple_gru and simple_lstm only (model kind %d)", m->kind);
    if (m->num_layers != 1)
        return fail(KWS_ERR_UNSUPPORTED, "dynamic-range int8 quantization covers one recurrent layer, not num_layers = %d", m->num_layers);
    if (m->feature_size < 1 || m->feature_size > KWS_QRNN_MAX_FEATURES)
        return fail(KWS_ERR_UNSUPPORTED, "dynamic-range int8 quantization covers feature_size 1..%d, not %d", KWS_QRNN_MAX_FEATURES, m->feature_size);
    if (m->n_features < 1 || m->n_features > KWS_QRNN_MAX_STEPS)
        return fail(KWS_ERR_UNSUPPORTED, "dynamic-range int8 quantization covers 1..%d steps, not %d", KWS_QRNN_MAX_STEPS, m->n_features);
    if (m->C < 2 || m->C > KWS_QUANT_MAX_CLASSES)
        return fail(KWS_ERR_UNSUPPORTED, "dynamic-range int8 quantization covers 2..%d classes, not %d", KWS_QUANT_MAX_CLASSES, m->C);
    return KWS_OK;
}

bool all_finite(const float *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// per-column symmetric MAX_ABS of W (K x N, row-major) in double: codes, and s_j rounded once to fp32 (0 for an all-zero column)
void quantize_columns(const float *W, int K, int N, int8_t *q, float *s)
{
    for (int j = 0; j < N; ++j) {
        double a = 0.0;
        for (int k = 0; k < K; ++k) a = std::max(a, std::fabs((double)W[(size_t)k * N + j]));
        const double sj = a / 127.0;
        s[j] = (float)sj;
        for (int k = 0; k < K; ++k)
            q[(size_t)k * N + j] = a == 0.0 ? 0 : (int8_t)std::min(127.0, std::max(-127.0, std::rint((double)W[(size_t)k * N + j] / sj)));
    }
}

int rnn_qforward(const kws_qmodel *q, const float *feat, int B, float *logits, float *probs, int32_t *argmax, hipStream_t s)
{
    QRnnArgs a{feat, B, q->T, q->F, q->C, q->rw, q->ru, q->fh, q->ep, logits, probs, argmax};
    if (q->kind == KWS_SIMPLE_GRU) {
        KWS_LAUNCH("qrnn_kernel<3>", qrnn_kernel<3>, dim3(blocks_for(B, 16)), dim3(64), 0, s, a);
    } else {
        KWS_LAUNCH("qrnn_kernel<4>", qrnn_kernel<4>, dim3(blocks_for(B, 16)), dim3(64), 0, s, a);
    }
    KWS_LAUNCH_CHECK("int8 recurrent forward");
    return KWS_OK;
}

}  // namespace q8
}  // namespace kws

using namespace kws;
using namespace kws::q8;

extern "C" {

int kws_quantize_simple_rnn(const kws_model *m, const float *params_host, kws_qsimple_rnn *q)
{
    int rc = check_rnn(m);
    if (rc) return rc;
    if (!params_host || !q) return fail(KWS_ERR_INVALID, "null argument");
    const int G = m->kind == KWS_SIMPLE_GRU ? 3 : 4, N = G * kRU, F = m->feature_size, C = m->C;
    const int nb = m->kind == KWS_SIMPLE_GRU ? 2 * N : N;
    const float *rk = params_host + m->o_rk, *ru = params_host + m->o_ru, *rb = params_host + m->o_rb;
    const float *hk = params_host + m->o_hk, *hb = params_host + m->o_hb;
    if (!all_finite(rk, (size_t)F * N) || !all_finite(ru, (size_t)kRU * N) || !all_finite(rb, nb) || !all_finite(hk, (size_t)kRU * C) ||
        !all_finite(hb, C))
        return fail(KWS_ERR_INVALID, "a weight or bias of the recurrent model is not finite");
    std::memset(q, 0, sizeof(*q));
    q->kind = m->kind;
    q->num_classes = C;
    q->n_steps = m->n_features;
    q->feature_size = F;
    q->method = KWS_QUANT_DYNAMIC;
    quantize_columns(rk, F, N, q->kernel, q->kernel_scale);
    quantize_columns(ru, kRU, N, q->recurrent_kernel, q->recurrent_scale);
    quantize_columns(hk, kRU, C, q->head_w, q->head_scale);
    std::memcpy(q->bias, rb, sizeof(float) * nb);
    std::memcpy(q->head_bias, hb, sizeof(float) * C);
    return KWS_OK;
}

int kws_qmodel_create_rnn(const kws_model *m, const kws_qsimple_rnn *q, kws_qmodel **out)
{
    if (!out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = check_rnn(m);
    if (rc) return rc;
    if (!q) return fail(KWS_ERR_INVALID, "null argument");
    if (q->kind != m->kind || q->num_classes != m->C || q->n_steps != m->n_features || q->feature_size != m->feature_size)
        return fail(KWS_ERR_INVALID, "quantized model (kind %d, C %d, T %d, F %d) does not match the model (kind %d, C %d, T %d, F %d)", q->kind,
                    q->num_classes, q->n_steps, q->feature_size, m->kind, m->C, m->n_features, m->feature_size);
    if (q->method != KWS_QUANT_DYNAMIC) return fail(KWS_ERR_INVALID, "a quantized recurrent model records method %d, not dynamic", q->method);
    const int G = m->kind == KWS_SIMPLE_GRU ? 3 : 4, N = G * kRU, F = m->feature_size, C = m->C;
    std::vector<float> ep(kQEpCount, 0.f);
    for (int j = 0; j < N; ++j) {
        ep[kQsW + j] = q->kernel_scale[j];
        ep[kQsU + j] = q->recurrent_scale[j];
        ep[kQb0 + j] = q->bias[j];
        ep[kQb1 + j] = G == 3 ? q->bias[N + j] : 0.f;
    }
    for (int j = 0; j < C; ++j) {
        ep[kQsH + j] = q->head_scale[j];
        ep[kQhb + j] = q->head_bias[j];
    }
    if (!all_finite(ep.data(), ep.size())) return fail(KWS_ERR_INVALID, "a scale or bias of the quantized model is not finite");
    std::vector<int8_t> fw, fu, fh;
    pack_frags(q->kernel, F, N, 1, 3 * G, fw);
    pack_frags(q->recurrent_kernel, kRU, N, 1, 3 * G, fu);
    pack_frags(q->head_w, kRU, C, 1, 3, fh);
    QBlob img;
    const size_t ow = img.put(fw.data(), fw.size()), ou = img.put(fu.data(), fu.size()), oh = img.put(fh.data(), fh.size()),
                 oe = img.put(ep.data(), sizeof(float) * ep.size());
    auto *qm = new kws_qmodel();
    qm->kind = m->kind;
    qm->C = C;
    qm->T = m->n_features;
    qm->F = F;
    const unsigned char *b = img.upload(qm);
    if (!b) { delete qm; return KWS_ERR_HIP; }
    qm->rw = reinterpret_cast<const i32x4 *>(b + ow);
    qm->ru = reinterpret_cast<const i32x4 *>(b + ou);
    qm->fh = reinterpret_cast<const i32x4 *>(b + oh);
    qm->ep = reinterpret_cast<const float *>(b + oe);
    *out = qm;
    return KWS_OK;
}

}  // extern "C"
