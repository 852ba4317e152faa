// csrc/kws_lstm.h -- LSTM(48, activation='tanh', dropout=0.2): the cell of the shared forward and BPTT kernels (kws_rnn_kernels.h;
// classifier/models/rnn.py:46-79).
//
// Keras LSTM semantics: kernel (F, 4u), recurrent_kernel (u, 4u), bias (4u); gate order i, f, c, o; recurrent_activation
// sigmoid; one input dropout mask per sample shared by all timesteps (the four gates share it, as Keras' fused
// implementation does):
//     a = x_t W + h U + b;  i = s(a_i);  f = s(a_f);  g = tanh(a_c);  o = s(a_o);  c' = f c + i g;  h' = o tanh(c')
// BPTT, per step and clip, with dh and dc carried backwards:
//   do = dh tanh(c');  dc += dh o (1 - tanh(c')^2)
//   da = [dc g i(1-i) | dc c_prev f(1-f) | dc i (1-g^2) | do o(1-o)]          (192 columns, tile G)
//   dW += x_t^T da;  dU += h_prev^T da;  db += sum da;  dh_prev = da U^T;  dc_prev = dc f
// (Round 2 ran both passes as three waves owning all four gates of their units: 68 / 128 dependent MFMAs per step per wave, 0.080 /
// 0.160 ms at B = 2048; the shared form 0.054 / 0.100 ms -- DESIGN.md section 5.)
#pragma once
#include "kws_rnn_kernels.h"

namespace kws {

constexpr int kLstmN = 4 * kGruU;          // 192 gate columns
constexpr int kLstmSave = 7;               // saved per (clip, step): h_prev, c_prev, i, f, g, o, tanh(c')

struct LstmCell {
    static constexpr int kN = kLstmN, kSave = kLstmSave;
    static constexpr const char *kFwdName = "lstm_fwd_kernel", *kBwdName = "lstm_bwd_kernel";

    // Forward: all twelve waves are product waves.  Pre-activation planes: i | f | c | o, one per gate with its bias.
    __device__ static __forceinline__ bool splits(int) { return false; }
    __device__ static __forceinline__ void fwd_bias(const float *__restrict__ bias, int, int col, float &bx, float &bh)
    {
        bx = bias[col];
        bh = 0.f;
    }
    // output (clip c, unit k) from the planes P and the state tile hc; cst: the cell state, in a register for the whole sequence
    __device__ static __forceinline__ float fwd_gate(const float *P, const float *hc, int c, int k, float &cst, float (&rec)[kLstmSave])
    {
        const float ig = sigmoidf_(P[c * kGruPS + k]), fg = sigmoidf_(P[(16 + c) * kGruPS + k]);
        const float gg = tanh_fast_(P[(32 + c) * kGruPS + k]), og = sigmoidf_(P[(48 + c) * kGruPS + k]);
        const float cp = cst, cn = fg * cp + ig * gg, tc = tanh_fast_(cn);
        const float hp = hc[c * kGruHS + k];
        cst = cn;
        rec[0] = hp; rec[1] = cp; rec[2] = ig; rec[3] = fg; rec[4] = gg; rec[5] = og; rec[6] = tc;
        return og * tc;
    }

    // Backward.  G planes g: da_i | da_f | da_c | da_o, all of them in every product; dh_prev is the product alone.
    // dcs: dL/dc of this (clip, unit), carried backwards.
    static constexpr bool kDhTerm = false;
    __device__ static __forceinline__ int gcol(int n) { return n; }
    __device__ static __forceinline__ float bwd_gate(const float (&sv)[kLstmSave], float dh, float &dcs, float (&g)[4])
    {
        const float cp = sv[1], ig = sv[2], fg = sv[3], gg = sv[4], og = sv[5], tc = sv[6];
        const float dc = dcs + dh * og * (1.f - tc * tc);
        const float gi = dc * gg * ig * (1.f - ig), gf = dc * cp * fg * (1.f - fg), gc = dc * ig * (1.f - gg * gg), go = dh * tc * og * (1.f - og);
        g[0] = gi; g[1] = gf; g[2] = gc; g[3] = go;
        dcs = dc * fg;
        return 0.f;
    }
    // Column sums of the G planes.  A plain array, not a struct: the compiler keeps the BPTT kernels' registers as they were this way.
    using BiasSums = float[4];
    __device__ static __forceinline__ void bias_add(float (&sbq)[4], const float (&g)[4]) { sbq[0] += g[0]; sbq[1] += g[1]; sbq[2] += g[2]; sbq[3] += g[3]; }
    __device__ static __forceinline__ void bias_write(float (&sbq)[4], float *db, int u, int lq)
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                  // lanes with equal li hold the same unit: reduce over lq
            sbq[q] += __shfl_xor(sbq[q], 16, 64);
            sbq[q] += __shfl_xor(sbq[q], 32, 64);
            if (lq == 0) atomicAdd(db + q * kGruU + u, sbq[q]);
        }
    }
};

}  // namespace kws
