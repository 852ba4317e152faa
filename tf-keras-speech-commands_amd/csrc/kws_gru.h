// csrc/kws_gru.h -- GRU(48, activation='linear', dropout=0.2): the cell of the shared forward and BPTT kernels (kws_rnn_kernels.h;
// classifier/models/rnn.py:34-35).
//
// Keras v2 GRU semantics (reset_after=True, bias (2,144), gate order z,r,h, recurrent_activation sigmoid, one input
// dropout mask per sample shared by all timesteps):
//     mx = x_t W + b0;  mh = h U + b1;  z = s(mx_z + mh_z);  r = s(mx_r + mh_r)
//     hh = mx_h + r * mh_h  (activation='linear': no tanh);   h' = z h + (1 - z) hh
// BPTT, per step and clip:
//   dz = dh (h_prev - hh); dhh = dh (1 - z); dr = dhh mh_h; dmh_h = dhh r; dz' = dz z(1-z); dr' = dr r(1-r)
//   dmx = [dz' dr' dhh]; dmh = [dz' dr' dmh_h];  dh_prev = dh z + dmh U^T
//   dW += x_t^T dmx; dU += h_prev^T dmh; db0 += sum dmx; db1 += sum dmh      (block partials -> float atomics)
#pragma once
#include "kws_rnn_kernels.h"

namespace kws {

constexpr int kGruN = 3 * kGruU;          // 144 gate columns
constexpr int kGruSave = 5;               // saved per (clip, step): h_prev, z, r, hh, mh_h

struct GruCell {
    static constexpr int kN = kGruN, kSave = kGruSave;
    static constexpr const char *kFwdName = "gru_fwd_kernel", *kBwdName = "gru_bwd_kernel";

    // Forward: nine product waves of the twelve.  Pre-activation planes: z | r | x-part of hh | h-part of hh.
    // z, r: one pre-activation with both biases; hh keeps its x-part (bias b0) and h-part (bias b1) apart: hh = mx_h + r * mh_h
    __device__ static __forceinline__ bool splits(int gate) { return gate >= 2; }
    __device__ static __forceinline__ void fwd_bias(const float *__restrict__ bias, int gate, int col, float &bx, float &bh)
    {
        bx = gate < 2 ? bias[col] + bias[kGruN + col] : bias[col];
        bh = gate < 2 ? 0.f : bias[kGruN + col];
    }
    // output (clip c, unit k) from the planes P and the state tile hc; no carried state
    __device__ static __forceinline__ float fwd_gate(const float *P, const float *hc, int c, int k, float &, float (&rec)[kGruSave])
    {
        const float z = sigmoidf_(P[c * kGruPS + k]), rg = sigmoidf_(P[(16 + c) * kGruPS + k]);
        const float mhh = P[(48 + c) * kGruPS + k];
        const float hh = P[(32 + c) * kGruPS + k] + rg * mhh;
        const float hp = hc[c * kGruHS + k];
        rec[0] = hp; rec[1] = z; rec[2] = rg; rec[3] = hh; rec[4] = mhh;
        return z * hp + (1.f - z) * hh;
    }

    // Backward.  G planes g: dz' | dr' | dhh | dmh_h.  dmx = planes 0-2 (the first 144 columns), dmh = planes 0, 1, 3, which gcol maps
    // the 144 product indices of dh_prev and dU to.  Returns the dh z that dh_prev takes besides the product.
    static constexpr bool kDhTerm = true;
    __device__ static __forceinline__ int gcol(int n) { return n < 96 ? n : n + kGruU; }
    __device__ static __forceinline__ float bwd_gate(const float (&sv)[kGruSave], float dh, float &, float (&g)[4])
    {
        const float hp = sv[0], z = sv[1], rg = sv[2], hh = sv[3], mhh = sv[4];
        const float dhh = dh * (1.f - z);
        const float gz = dh * (hp - hh) * z * (1.f - z), gr = dhh * mhh * rg * (1.f - rg), gm = dhh * rg;
        g[0] = gz; g[1] = gr; g[2] = dhh; g[3] = gm;
        return dh * z;
    }
    // Column sums of the G planes.  Four scalars, not an array: the compiler keeps the BPTT kernels' registers as they were this way.
    struct BiasSums {
        float sbz, sbr, sbh, sbm;
    };
    __device__ static __forceinline__ void bias_add(BiasSums &s, const float (&g)[4]) { s.sbz += g[0]; s.sbr += g[1]; s.sbh += g[2]; s.sbm += g[3]; }
    // db0 = sums of dmx = [dz' dr' dhh], db1 = sums of dmh = [dz' dr' dmh_h]; lanes with equal li hold the same unit: reduce over lq
    __device__ static __forceinline__ void bias_write(const BiasSums &s, float *db, int u, int lq)
    {
        float sbz = s.sbz, sbr = s.sbr, sbh = s.sbh, sbm = s.sbm;
        sbz += __shfl_xor(sbz, 16, 64); sbz += __shfl_xor(sbz, 32, 64);
        sbr += __shfl_xor(sbr, 16, 64); sbr += __shfl_xor(sbr, 32, 64);
        sbh += __shfl_xor(sbh, 16, 64); sbh += __shfl_xor(sbh, 32, 64);
        sbm += __shfl_xor(sbm, 16, 64); sbm += __shfl_xor(sbm, 32, 64);
        if (lq == 0) {
            atomicAdd(db + u, sbz);
            atomicAdd(db + kGruU + u, sbr);
            atomicAdd(db + 2 * kGruU + u, sbh);
            atomicAdd(db + kGruN + u, sbz);
            atomicAdd(db + kGruN + kGruU + u, sbr);
            atomicAdd(db + kGruN + 2 * kGruU + u, sbm);
        }
    }
};

}  // namespace kws
