// csrc/kws_rnn_kernels.h -- the forward and BPTT kernels of the recurrent layers, written once for both cells.
//
// rnn_fwd_kernel<Cell, ..> and rnn_bwd_kernel<Cell, ..> take a cell type (GruCell in kws_gru.h, LstmCell in kws_lstm.h) that carries only
// what differs between the two: the gate-column count N (144 / 192), the saved-values count, a product wave's bias and whether its x-part
// and h-part stay apart, the gate arithmetic of both passes (the forward hook reads its pre-activations and h_prev from LDS; every store
// and barrier is in the text below), the map from a product index to a column of the gradient tile, and the bias-gradient sums with their
// write-out.  Staging, LDS layout, wave roles, look-ahead fetch, products, barriers and the dU / dW / dx write-out are written once here.
// The hooks are __forceinline__ and keep the expressions, operand order and accumulator split of the two kernel pairs this replaced:
// outputs are bit-identical to those (profiles/rnn_cell_template_ab.txt).  The stores to the P and G planes stay in the template on
// purpose: from inside a hook the compiler formed their LDS addresses differently, and the BPTT kernels, which sit at the 168-VGPR cap,
// grew their scratch (profiles/rnn_cell_template_resources.txt has the figures to hold a change against).
//
// Forward.  Block = 16 clips x 12 waves.  Product wave w (w < N / 16) owns ONE 16-column tile of the N gate columns (gate w / 3 of hidden
// units 16 (w % 3) ..): 12 + KX MFMAs per step in three accumulation chains, its W / U fragments in registers for the whole sequence.  The
// pre-activations go through an LDS tile, and after a barrier each of the 768 threads applies the gate arithmetic to ONE of the 16 x 48
// outputs.  h ping-pongs through a 2 x 16 x 48 LDS tile; the clip tile's features are staged in LDS once.  Two barriers per step.
//
// BPTT.  Per step (t = T-1 .. 0) and 16-clip tile, nine waves: waves 0-2 carry the recurrence (gate gradients G of their 16 hidden units
// -> LDS, then dh_prev = G U^T), waves 3-5 and 6-8 take the two weight-gradient products of the SAME step (dU, dW: none of them feeds the
// recurrence) from the G / h_prev / x tiles in LDS, between the same two barriers.  For the GRU the step's critical path is then 36 MFMAs
// instead of 96 (three waves doing everything: 109 us at B = 2048; six waves, dU + dW together: 90 us).
// Stacked models add two things, both compiled out of the one-layer kernel:
//   DSEQ (every layer but the last): the dh entering step t is the recurrent dh plus dseq_in[b, t, :], the input gradient written by the
//        layer above; the gradient of the last state is zero and dh_last is not read.  The values ride in the look-ahead of the saved ones.
//   DX   (every layer but the first; F == 48): dx_t = G_t[:, :N] W^T times the layer's dropout mask goes to dx_out (B, T, 48).  Three more
//        waves (9-11) hold W^T's fragments in registers and take the N / 4 MFMAs per step from the G tile between the same two barriers
//        as the dU / dW waves: nothing of it is on the recurrence waves' chain.
#pragma once
#include "kws_device.h"

namespace kws {

// 1 / (1 + e^-x) on the hardware exp2 / reciprocal (each within ~1 ulp; the library expf + IEEE division cost ~60 instructions per gate value,
// a third of a recurrent step that one wave per SIMD issues alone).  e^-x overflows to inf for x < -88 -> 0, underflows to 0 for x > 88 -> 1.
__device__ __forceinline__ float sigmoidf_(float x)
{
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

// tanh(x) = (1 - e^-2|x|) / (1 + e^-2|x|) with the sign of x, on the same two hardware instructions (absolute error ~2e-7; the form
// 2 sigmoid(2x) - 1 cancels for small x)
__device__ __forceinline__ float tanh_fast_(float x)
{
    const float e = __builtin_amdgcn_exp2f(-2.88539008177792681f * fabsf(x));
    const float t = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e);
    return copysignf(t, x);
}

constexpr int kGruU = 48;                 // recurrent_units (classifier/model.py:27)
constexpr int kGruHS = 50;                // LDS row stride of a 48-wide state tile (== 18 mod 32: conflict-free A reads)
constexpr int kGruGS = 210;               // row stride of the 192-wide gradient tile (== 18 mod 32)
constexpr int kGruPS = 50;                // row stride of a pre-activation plane
constexpr int kGruFwdThreads = 768;       // twelve waves: the gate arithmetic is one output per thread
constexpr int kGruBwdThreads = 576, kGruBwdDxThreads = 768;

__host__ __device__ inline int gru_xstride(int T, int F)
{
    int s = T * F;
    while (s % 32 != 18) ++s;
    return s;
}

inline size_t gru_fwd_smem(int T, int F) { return sizeof(float) * (size_t)(16 * gru_xstride(T, F) + 2 * 16 * kGruHS + 4 * 16 * kGruPS); }
inline size_t gru_bwd_smem(int T, int F)
{
    return sizeof(float) * (size_t)(16 * gru_xstride(T, F) + 16 * kGruGS + 16 * kGruHS + 2 * 16 * kGruHS);
}

// stage the 16-clip feature tile (with the per-sample input dropout mask) into LDS
__device__ __forceinline__ void gru_stage_x(const float *__restrict__ feat, float *xs, int b0, int B, int T, int F, int XS,
                                            float drop_rate, uint32_t slo, uint32_t shi)
{
    const int TF = T * F;
    for (int i = threadIdx.x; i < 16 * TF; i += blockDim.x) {
        const int c = i / TF, e = i % TF, b = b0 + c;
        float v = 0.f;
        if (b < B) {
            v = feat[(long)b * TF + e];
            if (drop_rate > 0.f)
                v = dropout_keep(slo, shi, (uint32_t)(b * F + e % F), drop_rate) ? v / (1.f - drop_rate) : 0.f;
        }
        xs[c * XS + e] = v;
    }
}

// SEQ (a layer of a stacked model that is not the last one): h_t of every step goes to seq_out (B, T, 48), the input of the layer above,
// and h_out is not written.
template <class Cell, int KX, bool SAVE, bool SEQ = false>
__global__ __launch_bounds__(kGruFwdThreads) void rnn_fwd_kernel(const float *__restrict__ feat, const float *__restrict__ Wk,
                                                                  const float *__restrict__ Uk, const float *__restrict__ bias,
                                                                  float *__restrict__ h_out, float *__restrict__ saved, int B, int T,
                                                                  int F, float drop_rate, uint32_t slo, uint32_t shi, float *__restrict__ zero_buf = nullptr, long zero_n = 0,
                                                                  float *__restrict__ seq_out = nullptr)
{
    constexpr int N = Cell::kN;
    // training: the gradient buffer of the backward pass that follows is cleared here (zero_n floats over the whole grid) instead of by a
    // memset node on the step's chain
    if (zero_buf)
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < zero_n; i += (long)gridDim.x * blockDim.x) zero_buf[i] = 0.f;
    extern __shared__ float gsm[];
    const int XS = gru_xstride(T, F);
    float *xs = gsm;                       // [16][XS]
    float *hs = gsm + 16 * XS;             // [2][16][kGruHS]
    float *P = hs + 2 * 16 * kGruHS;       // [4][16][kGruPS]: the cell's pre-activation planes (biases included)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    const bool mm = N / 16 == kGruFwdThreads / 64 || wave < N / 16;          // product waves
    const int gate = mm ? wave / 3 : 0, b0 = blockIdx.x * 16, u = 16 * (wave % 3) + li, col = gate * kGruU + u;

    float wg[KX], ug[12];
#pragma unroll
    for (int j = 0; j < KX; ++j) {
        const int k = 4 * j + lq;
        wg[j] = k < F ? Wk[k * N + col] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) ug[j] = Uk[(4 * j + lq) * N + col];
    float bx, bh;                          // the wave's bias: of its pre-activation, or of its x-part and h-part where the cell splits them
    Cell::fwd_bias(bias, gate, col, bx, bh);

    gru_stage_x(feat, xs, b0, B, T, F, XS, drop_rate, slo, shi);
    for (int i = threadIdx.x; i < 2 * 16 * kGruHS; i += kGruFwdThreads) hs[i] = 0.f;
    __syncthreads();

    const int ec = threadIdx.x / kGruU, ek = threadIdx.x - ec * kGruU;          // this thread's output (clip, unit) in the gate phase
    float carry = 0.f;                                                          // what the cell carries forwards besides h (the LSTM's c)
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        const float *hc = hs + cur * 16 * kGruHS;
        if (mm) {
            float xa[KX], ha[12];
#pragma unroll
            for (int j = 0; j < KX; ++j) {
                const int k = 4 * j + lq;
                xa[j] = k < F ? xs[li * XS + t * F + k] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) ha[j] = hc[li * kGruHS + 4 * j + lq];
            // x-part and two halves of the h-part in separate accumulators: three short dependent chains instead of one of 12 + KX
            f32x4 ax = {0.f, 0.f, 0.f, 0.f}, ah0 = ax, ah1 = ax;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (j < KX) ax = mfma16(xa[j], wg[j], ax);
                ah0 = mfma16(ha[j], ug[j], ah0);
                ah1 = mfma16(ha[6 + j], ug[6 + j], ah1);
            }
#pragma unroll
            for (int j = 6; j < KX; ++j) ax = mfma16(xa[j], wg[j], ax);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * lq + r;
                const float hsum = ah0[r] + ah1[r];
                if (!Cell::splits(gate)) P[(gate * 16 + c) * kGruPS + u] = (ax[r] + hsum) + bx;
                else {                     // the GRU's hh: x-part and h-part apart, in planes 2 and 3
                    P[(2 * 16 + c) * kGruPS + u] = ax[r] + bx;
                    P[(3 * 16 + c) * kGruPS + u] = hsum + bh;
                }
            }
        }
        __syncthreads();
        float *hn = hs + (cur ^ 1) * 16 * kGruHS;
        {
            float rec[Cell::kSave];                                             // what the cell saves for its BPTT, h_prev first
            const float hnew = Cell::fwd_gate(P, hc, ec, ek, carry, rec);
            hn[ec * kGruHS + ek] = hnew;
            if (SEQ && b0 + ec < B) seq_out[((long)(b0 + ec) * T + t) * kGruU + ek] = hnew;
            if (SAVE && b0 + ec < B) {
                float *sv = saved + (((long)(b0 + ec) * T + t) * Cell::kSave) * kGruU + ek;
#pragma unroll
                for (int q = 0; q < Cell::kSave; ++q) sv[q * kGruU] = rec[q];
            }
        }
        cur ^= 1;
        __syncthreads();
    }
    if (!SEQ && b0 + ec < B) h_out[(long)(b0 + ec) * kGruU + ek] = hs[cur * 16 * kGruHS + ec * kGruHS + ek];
}

template <class Cell, int KX, bool DSEQ = false, bool DX = false>
__global__ __launch_bounds__(DX ? kGruBwdDxThreads : kGruBwdThreads) void rnn_bwd_kernel(const float *__restrict__ feat, const float *__restrict__ Uk,
                                                                  const float *__restrict__ saved, const float *__restrict__ dh_last,
                                                                  float *__restrict__ dW, float *__restrict__ dU, float *__restrict__ db,
                                                                  int B, int T, int F, float drop_rate, uint32_t slo, uint32_t shi,
                                                                  const float *__restrict__ dseq_in = nullptr,
                                                                  const float *__restrict__ Wk = nullptr, float *__restrict__ dx_out = nullptr)
{
    constexpr int N = Cell::kN, NF = N / 4, NTL = N / 16, NS = Cell::kSave;      // gate columns, their K = 4 fragments and 16-column tiles
    constexpr int NT = DX ? kGruBwdDxThreads : kGruBwdThreads;
    constexpr int MTW = (KX * 4 + 15) / 16;            // 16-row tiles covering the F input features
    constexpr int WT = (MTW * NTL + 2) / 3;            // dW tiles per wave
    extern __shared__ float gsm[];
    const int XS = gru_xstride(T, F);
    float *xs = gsm;                                   // [16][XS]
    float *G = gsm + 16 * XS;                          // [16][kGruGS]: the cell's four gate-gradient planes
    float *Hp = G + 16 * kGruGS;                       // [16][kGruHS] h_prev of the step
    float *dhs = Hp + 16 * kGruHS;                     // [2][16][kGruHS]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    const bool rec = wave < 3;                         // recurrence waves; waves 3-5 accumulate dU, waves 6-8 dW
    const bool do_u = wave >= 3 && wave < 6;
    const int w3 = wave % 3;
    const int b0 = blockIdx.x * 16, u = 16 * w3 + li;

    gru_stage_x(feat, xs, b0, B, T, F, XS, drop_rate, slo, shi);
    for (int i = threadIdx.x; i < 16 * kGruU; i += NT) {
        const int c = i / kGruU, k = i % kGruU;
        dhs[c * kGruHS + k] = (!DSEQ && b0 + c < B) ? dh_last[(long)(b0 + c) * kGruU + k] : 0.f;
    }
    __syncthreads();

    if (rec) {
        float ut[NF];                                  // B fragments of U^T restricted to the columns that feed dh_prev
#pragma unroll
        for (int j = 0; j < NF; ++j) ut[j] = Uk[u * N + 4 * j + lq];
        typename Cell::BiasSums sb = {};               // bias partials of unit u over this lane's four clips, one per G plane
        float carry[4] = {0.f, 0.f, 0.f, 0.f};         // what the cell carries backwards besides dh, per clip (the LSTM's dc)
        // the step's saved forward values (of this lane's four clips) come from global memory: they are requested one step AHEAD, under the
        // previous step's products, by unconditional loads on clamped (clip, step) addresses, masked afterwards
        float svn[4][NS], dsn[4] = {0.f, 0.f, 0.f, 0.f};
        const float *svbase[4], *dsbase[4];
        float svmask[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 4 * lq + r;
            const bool in = b0 + c < B;
            svbase[r] = saved + ((long)(in ? b0 + c : b0) * T * NS) * kGruU + u;
            dsbase[r] = DSEQ ? dseq_in + ((long)(in ? b0 + c : b0) * T) * kGruU + u : nullptr;
            svmask[r] = in ? 1.f : 0.f;
        }
        auto fetch_saved = [&](int t) {
            const int tc = t >= 0 ? t : 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *sv = svbase[r] + (long)tc * NS * kGruU;
#pragma unroll
                for (int q = 0; q < NS; ++q) svn[r][q] = sv[q * kGruU] * svmask[r];
                if (DSEQ) dsn[r] = dsbase[r][(long)tc * kGruU] * svmask[r];
            }
        };
        fetch_saved(T - 1);
        int cur = 0;
        for (int t = T - 1; t >= 0; --t) {
            const float *dc = dhs + cur * 16 * kGruHS;
            float dht[4], svc[4][NS], dsc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int q = 0; q < NS; ++q) svc[r][q] = svn[r][q];
                dsc[r] = dsn[r];
            }
            fetch_saved(t - 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * lq + r;
                const float dh = DSEQ ? dc[c * kGruHS + u] + dsc[r] : dc[c * kGruHS + u];
                float g[4];
                dht[r] = Cell::bwd_gate(svc[r], dh, carry[r], g);
                G[c * kGruGS + u] = g[0];
                G[c * kGruGS + kGruU + u] = g[1];
                G[c * kGruGS + 2 * kGruU + u] = g[2];
                G[c * kGruGS + 3 * kGruU + u] = g[3];
                Hp[c * kGruHS + u] = svc[r][0];
                Cell::bias_add(sb, g);   // bias gradients: column sums of G (clips past B contribute zeros)
            }
            __syncthreads();                           // G, Hp of step t complete (the other waves start their products)
            // dh_prev = G U^T (+ the cell's direct term): operands in one batch of LDS reads, three accumulation chains
            float ga[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) ga[j] = G[li * kGruGS + Cell::gcol(4 * j + lq)];
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0;
#pragma unroll
            for (int j = 0; j < NF / 3; ++j) {
                acc0 = mfma16(ga[3 * j], ut[3 * j], acc0);
                acc1 = mfma16(ga[3 * j + 1], ut[3 * j + 1], acc1);
                acc2 = mfma16(ga[3 * j + 2], ut[3 * j + 2], acc2);
            }
            float *dn = dhs + (cur ^ 1) * 16 * kGruHS;
#pragma unroll
            for (int r = 0; r < 4; ++r) dn[(4 * lq + r) * kGruHS + u] = Cell::kDhTerm ? (acc0[r] + acc1[r]) + acc2[r] + dht[r] : (acc0[r] + acc1[r]) + acc2[r];
            cur ^= 1;
            __syncthreads();                           // dh of step t-1 complete; G / Hp may be overwritten
        }
        Cell::bias_write(sb, db, u, lq);
    } else if (DX && wave >= 9) {
        // dx_t[clip][f] = sum_n G_t[clip][n] W[f][n] over the first N columns of G; this wave owns f = 16 w3 + li
        float wt[NF], mk[4];
#pragma unroll
        for (int j = 0; j < NF; ++j) wt[j] = u < F ? Wk[u * N + 4 * j + lq] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 4 * lq + r;
            mk[r] = 1.f;
            if (drop_rate > 0.f && b < B && u < F) mk[r] = dropout_keep(slo, shi, (uint32_t)(b * F + u), drop_rate) ? 1.f / (1.f - drop_rate) : 0.f;
        }
        for (int t = T - 1; t >= 0; --t) {
            __syncthreads();                           // G of step t complete
            float ga[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) ga[j] = G[li * kGruGS + 4 * j + lq];
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0;
#pragma unroll
            for (int j = 0; j < NF / 3; ++j) {
                acc0 = mfma16(ga[3 * j], wt[3 * j], acc0);
                acc1 = mfma16(ga[3 * j + 1], wt[3 * j + 1], acc1);
                acc2 = mfma16(ga[3 * j + 2], wt[3 * j + 2], acc2);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + 4 * lq + r;
                if (b < B && u < F) dx_out[((long)b * T + t) * F + u] = ((acc0[r] + acc1[r]) + acc2[r]) * mk[r];
            }
            __syncthreads();                           // the recurrence waves may overwrite G
        }
    } else {
        f32x4 accU[NTL], accW[WT];
#pragma unroll
        for (int i = 0; i < NTL; ++i) accU[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < WT; ++i) accW[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int t = T - 1; t >= 0; --t) {
            __syncthreads();                           // G, Hp of step t complete
            // every operand of the step's products in one batch of LDS reads, then the products from registers
            if (do_u) {
                float hv[4], gu[NTL][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) hv[j] = Hp[(4 * j + lq) * kGruHS + u];
#pragma unroll
                for (int nt = 0; nt < NTL; ++nt) {
                    const int gcol = Cell::gcol(16 * nt + li);
#pragma unroll
                    for (int j = 0; j < 4; ++j) gu[nt][j] = G[(4 * j + lq) * kGruGS + gcol];
                }
                // dU[16w + ..][:] += h_prev^T G (reduction index = clip); j outside: consecutive MFMAs write different accumulators
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int nt = 0; nt < NTL; ++nt) accU[nt] = mfma16(hv[j], gu[nt][j], accU[nt]);
            } else {
                float gw[WT][4], xa[WT][4];
#pragma unroll
                for (int i = 0; i < WT; ++i) {
                    const int tile = w3 + 3 * i, tl = tile < MTW * NTL ? tile : 0;
                    const int mt = tl / NTL, nt = tl % NTL, f = 16 * mt + li;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        gw[i][j] = G[(4 * j + lq) * kGruGS + 16 * nt + li];
                        xa[i][j] = f < F ? xs[(4 * j + lq) * XS + t * F + f] : 0.f;
                    }
                }
                // dW tiles (feature rows x the first N columns of G), dealt round-robin to the three waves; tiles past the end multiply
                // tile-0 operands into an accumulator that is never stored
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < WT; ++i) accW[i] = mfma16(xa[i][j], gw[i][j], accW[i]);
            }
            __syncthreads();                           // the recurrence waves may overwrite G / Hp
        }
        // D layout: row = 4*lq + r, col = li
        if (do_u) {
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) atomicAdd(dU + (16 * w3 + 4 * lq + r) * N + 16 * nt + li, accU[nt][r]);
        }
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            const int tile = w3 + 3 * i;
            if (!do_u && tile < MTW * NTL) {
                const int mt = tile / NTL, nt = tile % NTL;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * mt + 4 * lq + r;
                    if (f < F) atomicAdd(dW + f * N + 16 * nt + li, accW[i][r]);
                }
            }
        }
    }
}

}  // namespace kws
