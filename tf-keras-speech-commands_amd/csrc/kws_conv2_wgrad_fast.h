// csrc/kws_conv2_wgrad_fast.h -- conv2's split-precision weight gradient for the default map (15 x 10, 16 -> 32 channels), one WAVE per clip.
//
// kws_conv.h: conv_wgrad_clip_bf16_kernel<true> gives a clip to a block of four waves: all 256 threads form dz2 and split it and x into bf16
// planes, barrier, the four waves (column tile x tap parity) read the planes back, barrier -- staging and products never overlap inside a
// block, the two waves of a tap parity read the same x fragments, and the map size is a runtime value.  Here a wave owns whole clips and
// a private 12.75 KB of LDS, so the kernel has no barrier in front of its epilogue: while one wave of a SIMD splits and stores, the other
// one runs its products.  The map is a template parameter:
//   - a k-step is RS = 3 map rows (30 pixels + 2 pixels whose dz rows stay zero), so the clip is H / 3 = 5 k-steps with nothing but the two
//     pad pixels wasted, the same count as the 32-pixel steps of the block kernel;
//   - dz of ONE k-step lives in LDS ([plane][channel half][32 pixels][16 channels] bf16, 6 KB), formed by the same expression as in the
//     block kernel from the routed gradient (bn.gw / bn.arg) and z2, coefficients from the accumulator set (bn_bwd_k_from_acc);
//   - x lives in a ring of 2 RS = 6 haloed rows per plane ([plane][row slot][W + 2][16 channels], 6.75 KB): step k reads haloed rows
//     3k .. 3k + 4 and the staging behind it writes the three rows the next step adds, into the slots the step before last has left.  The slot of
//     (pixel row, kh) depends on the lane only through a table of 2 parities x 3 kh x 2 reads computed once; kw and the plane are immediates;
//   - the wave keeps all 9 taps x 2 column tiles in 18 accumulators: every x fragment is read once per clip and k-step, every dz fragment
//     once per k-step; the six partial products of the two column tiles of a tap alternate, so consecutive MFMAs are independent;
//   - the raw data of the next k-step (x rows, z2, routed gradient, element indices: 12 loads per lane) is fetched in front of the products
//     of the current one and split / stored behind them.
// LDS traffic of one wave is in order, so a compiler fence at wavefront scope is all that separates its stores from its transposing reads.
// The four waves of a block meet once, to add their tiles in LDS in front of the contiguous float atomics (the block kernel's epilogue).
// Same arithmetic per product (split_bf16, the six products of mfma_bf16x6 in its order, fp32 accumulation); only the order in which pixels
// enter an accumulator differs.  Chosen by plan_cnn (wgrad2_fast); every other geometry, deterministic mode and graph capture keep the
// block kernel.
#pragma once
#include "kws_cnn_shape.h"   // kW2fH x kW2fW, the map the kernel is instantiated for: plan_cnn reads it

namespace kws {

template <int H, int W>
struct Conv2WgradFast {
    static constexpr int CIN = 16, COUT = 32, RS = 3, KS = H / RS, RING = 2 * RS, WP = W + 2, HW = H * W, KP = RS * W;
    static constexpr int RB = WP * 32, XPL = RING * RB, DPL = 32 * 32;      // bytes: haloed x row, x plane, dz (plane, channel half)
    static constexpr int XBYTES = 3 * XPL, WAVE_BYTES = XBYTES + 6 * DPL, BYTES = 4 * WAVE_BYTES;
    static constexpr int NX4 = (RS + 1) * W * 4;                   // float4 of the largest x staging (step 0: four rows)
    static_assert(H % RS == 0 && KS >= 2 && W % 2 == 0 && KP <= 32 && KP > 24, "a k-step is three whole map rows, 25..32 pixels");
    static_assert(NX4 <= 192 && WAVE_BYTES % 16 == 0, "three float4 of x per lane");
    static_assert(BYTES >= 4 * 9 * CIN * COUT, "the block's tile fits the staging space");
    // persistent grid: at most max_blocks blocks, every wave with the same number of clips (+- the remainder of B)
    static unsigned grid(int B, int max_blocks) { const int cpw = (B + 4 * max_blocks - 1) / (4 * max_blocks); return (unsigned)((B + 4 * cpw - 1) / (4 * cpw)); }
};

template <int H, int W>
__global__ __launch_bounds__(256, 2) void conv2_wgrad_fast_kernel(const float *__restrict__ x, float *__restrict__ dw, int B, BnBwdArgs bn)
{
    using G = Conv2WgradFast<H, W>;
    constexpr int CIN = G::CIN, COUT = G::COUT, RS = G::RS, KS = G::KS, RING = G::RING, HW = G::HW, KP = G::KP;
    constexpr int RB = G::RB, XPL = G::XPL, DPL = G::DPL, Wp = W / 2, NWIN = (H / 2) * Wp, F4 = COUT / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctile[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, lq = lane >> 4;
    unsigned char *Xs = ctile + wave * G::WAVE_BYTES, *Ds = Xs + G::XBYTES;
#pragma unroll
    for (int j = 0; j < (G::WAVE_BYTES / 16 + 63) / 64; ++j) {      // column halos and the pad pixels of dz stay zero from here on
        const int i = lane + 64 * j;
        if (i < G::WAVE_BYTES / 16) reinterpret_cast<f32x4 *>(Xs)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // BatchNorm coefficients of the 4 channels of every dz float4 a lane stages (c4 = lane % 8): derived as in the block kernel, then kept
    // in LDS ([gi | mean | inv | k2 | k3][COUT]) and read back while staging, so that they hold no registers during the products
    __shared__ __attribute__((aligned(16))) float coef[5][COUT];
    const int c4 = lane & (F4 - 1), l8 = lane >> 3;
    {
        f32x4 gi, mean, inv;
        float k2[4], k3[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            inv[e] = bn.inv[c]; gi[e] = bn.gamma[c] * inv[e]; mean[e] = bn.mean[c];
        }
        bn_bwd_k_from_acc(bn, COUT, c4, false, k2, k3);
        if (threadIdx.x < F4) {
            *reinterpret_cast<f32x4 *>(&coef[0][4 * c4]) = gi;
            *reinterpret_cast<f32x4 *>(&coef[1][4 * c4]) = mean;
            *reinterpret_cast<f32x4 *>(&coef[2][4 * c4]) = inv;
            *reinterpret_cast<f32x4 *>(&coef[3][4 * c4]) = (f32x4){k2[0], k2[1], k2[2], k2[3]};
            *reinterpret_cast<f32x4 *>(&coef[4][4 * c4]) = (f32x4){k3[0], k3[1], k3[2], k3[3]};
        }
        __syncthreads();
    }

    // transposing reads: lane 4q + pp of a 16-lane group supplies the row of pixel q, channels 4pp..4pp+3; group lq takes pixels
    // 4 lq + q (first read) and 16 + 4 lq + q (second read) of the k-step.  Pad pixels: x row of pixel 0 (finite), their dz rows are zero.
    int xa[2][3][2], da[2];
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int pq = 16 * rd + 4 * lq + (li >> 2);
        const bool ok = pq < KP;
        const int ly = ok ? pq / W : 0, lx = ok ? pq - ly * W : 0;
        da[rd] = pq * 32 + (li & 3) * 8;
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) xa[par][kh][rd] = ((RS * par + ly + kh) % RING) * RB + lx * 32 + (li & 3) * 8;
    }
    // staging: dz float4 j of a k-step is (pixel l8 + 8 j, channels 4 c4 ..), x float4 j is element lane + 64 j of the rows being added
    int dly[4], dlx[4], xry[3], xof[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int pix = l8 + 8 * j; dly[j] = pix / W; dlx[j] = pix - dly[j] * W; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { const int i = lane + 64 * j, xp = i >> 2; xry[j] = xp / W; xof[j] = (xp - xry[j] * W + 1) * 32 + (i & 3) * 8; }
    const int dso = ((c4 >> 2) * 32 + l8) * 32 + (c4 & 3) * 8;

    auto frag = [&](const unsigned char *p0, const unsigned char *p1) -> bf16x8 {
        union { struct { s16x4 lo, hi; } s; bf16x8 v; } u;
        u.s.lo = lds_read_tr16(p0);
        u.s.hi = lds_read_tr16(p1);
        return u.v;
    };

    f32x4 acc[9][2];                                               // dW[tap][ci = 4 lq + r][co = 16 nt + li]
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t][0] = acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 rx[3], rz[4], rg[4];                                     // the next k-step's raw data
    unsigned ra[4];
    // x rows added in front of step k: map rows first(k) .. first(k) + rows(k) - 1 (step 0 brings row 0 along, the last step has the bottom halo)
    auto first = [](int k) { return k == 0 ? 0 : RS * k + 1; };
    auto rows = [&](int k) { return k == 0 ? RS + 1 : (H - first(k) < RS ? H - first(k) : RS); };
    auto load = [&](int k, long b) {
        const int nx4 = rows(k) * W * 4;
        const f32x4 *xs = reinterpret_cast<const f32x4 *>(x + (b * HW + first(k) * W) * CIN);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = lane + 64 * j;
            if (64 * j < nx4) rx[j] = i < nx4 ? xs[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const f32x4 *zs = reinterpret_cast<const f32x4 *>(bn.z + (b * HW + KP * k) * COUT);
        const f32x4 *gws = reinterpret_cast<const f32x4 *>(bn.gw) + b * NWIN * F4;
        const unsigned *ars = reinterpret_cast<const unsigned *>(bn.arg) + b * NWIN * F4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = RS * k + dly[j];
            const bool ok = l8 + 8 * j < KP, in = ok && y < 2 * (H / 2);
            const int q = in ? ((y >> 1) * Wp + (dlx[j] >> 1)) * F4 + c4 : 0;
            rg[j] = gws[q];
            ra[j] = ars[q];
            rz[j] = ok ? zs[lane + 64 * j] : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto put = [&](unsigned char *d, int plane_bytes, f32x4 v) {
        bf16x4 h, m, l;
        split_bf16(v, h, m, l);
        *reinterpret_cast<bf16x4 *>(d) = h;
        *reinterpret_cast<bf16x4 *>(d + plane_bytes) = m;
        *reinterpret_cast<bf16x4 *>(d + 2 * plane_bytes) = l;
    };
    auto zero_row = [&](int slot) {                                // the interior of a halo row in the three planes: 3 x W x 32 bytes
        if (lane < 3 * W * 2)
            *reinterpret_cast<f32x4 *>(Xs + (lane / (2 * W)) * XPL + slot * RB + 32 + (lane % (2 * W)) * 16) = (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    auto stage = [&](int k) {
        const int nx4 = rows(k) * W * 4, s0 = (first(k) + 1) % RING;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = lane + 64 * j;
            if (64 * j < nx4 && i < nx4) {
                int slot = s0 + xry[j];
                slot -= slot >= RING ? RING : 0;
                put(Xs + slot * RB + xof[j], XPL, rx[j]);
            }
        }
        if (k == 0) zero_row(0);
        if (k == KS - 1) zero_row((H + 1) % RING);
        const f32x4 gi = *reinterpret_cast<const f32x4 *>(&coef[0][4 * c4]), mean = *reinterpret_cast<const f32x4 *>(&coef[1][4 * c4]),
                    inv = *reinterpret_cast<const f32x4 *>(&coef[2][4 * c4]), k2 = *reinterpret_cast<const f32x4 *>(&coef[3][4 * c4]),
                    k3 = *reinterpret_cast<const f32x4 *>(&coef[4][4 * c4]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l8 + 8 * j < KP) {
                const int y = RS * k + dly[j], ce = (y & 1) * 2 + (dlx[j] & 1);
                const bool in = y < 2 * (H / 2);
                f32x4 v = rg[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {                      // g of this element from its window's routed value, then BatchNorm backward
                    const float g = (in && (int)((ra[j] >> (8 * e)) & 0xFFu) == ce) ? v[e] : 0.f;
                    v[e] = gi[e] * (g - k2[e] - (rz[j][e] - mean[e]) * inv[e] * k3[e]);
                }
                put(Ds + dso + j * 8 * 32, 2 * DPL, v);
            }
        }
    };
    auto products = [&](int k) {
        const int par = k & 1;
        bf16x8 bfr[2][3];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int p = 0; p < 3; ++p) bfr[nt][p] = frag(Ds + (2 * p + nt) * DPL + da[0], Ds + (2 * p + nt) * DPL + da[1]);
        auto xfrag = [&](int tap, bf16x8 (&a)[3]) {
            const int kh = tap / 3, kw = tap % 3;
#pragma unroll
            for (int p = 0; p < 3; ++p) a[p] = frag(Xs + p * XPL + kw * 32 + xa[par][kh][0], Xs + p * XPL + kw * 32 + xa[par][kh][1]);
        };
        // the x fragments of tap + 1 are read in front of the products of tap; the scheduling barriers keep the reads of later taps (and
        // with them 100 more live registers) from being hoisted to the head of the unrolled step
        bf16x8 a[2][3];
        xfrag(0, a[0]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap + 1 < 9) xfrag(tap + 1, a[(tap + 1) & 1]);
            // mfma_bf16x6's six products, small terms first, alternating between the two column tiles
            constexpr int pa[6] = {1, 2, 0, 1, 0, 0}, pb[6] = {1, 0, 2, 0, 1, 0};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                acc[tap][0] = mfma_bf16(a[tap & 1][pa[i]], bfr[0][pb[i]], acc[tap][0]);
                acc[tap][1] = mfma_bf16(a[tap & 1][pa[i]], bfr[1][pb[i]], acc[tap][1]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    const long stride = 4L * gridDim.x;
    long b = 4L * blockIdx.x + wave;                               // wave-uniform
    if (b < B) {
        load(0, b);
        stage(0);
    }
    for (; b < B; b += stride) {
        // the staging tables are opaque once per clip: everything derived from them for the five unrolled steps (window indices, ring slots)
        // is then a few vector operations per step instead of ~100 loop-invariant registers, which the kernel does not have
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(dly[j]), "+v"(dlx[j]));
#pragma unroll
        for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(xry[j]), "+v"(xof[j]));
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const bool wrap = k == KS - 1;
            const int nk = wrap ? 0 : k + 1;
            const long nb = wrap ? b + stride : b;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // this step's stores are in front of its reads (one wave: LDS is in order)
            if (nb < B) load(nk, nb);                              // in flight under the products
            __builtin_amdgcn_sched_barrier(0);
            products(k);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // ... and its reads in front of the next step's stores
            if (nb < B) stage(nk);
        }
    }

    // add the four waves' 9 x 16 x 32 tiles in LDS (reusing the staging space), then contiguous atomics
    float *red = reinterpret_cast<float *>(ctile);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float *p = red + (tap * CIN + 4 * lq + r) * COUT + 16 * nt + li;
                        *p = w == 0 ? acc[tap][nt][r] : *p + acc[tap][nt][r];
                    }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 9 * CIN * COUT; idx += 256) atomicAdd(dw + idx, red[idx]);
}

}  // namespace kws
