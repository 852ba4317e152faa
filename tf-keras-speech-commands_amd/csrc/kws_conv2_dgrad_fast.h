// csrc/kws_conv2_dgrad_fast.h -- conv2's split-precision data gradient for the default map (15 x 10, 32 -> 16 channels), one block per clip.
//
// kws_conv.h: conv_dgrad_clip_bf16_kernel<true, true, false> takes the map size as kernel arguments: every staged float4 divides by the
// runtime width, the four pixels of a pool window each load the window's routed gradient and index word again, and the BatchNorm
// coefficients and one clip of raw data (45 registers) stay in registers for the whole kernel.  Here the map is a template parameter:
//   - staging is WINDOW-major: a thread's unit is (pool window, four channels).  It loads the window's routed gradient (bn.gw) and its
//     index word (bn.arg) once and the four pixels' z2, forms the four dz2 float4 by the block kernel's expression, splits them and
//     stores the bf16 planes.  The first 256 / 8 = 32 windows are one unit per thread; what is left -- the last windows and the rows
//     below the last pool window (row 14 of 15: its g is zero, its dz2 is not) -- is cut into single pixels, spread over the four waves
//     (at 15 x 10: 12 + 10 pixels, 6 or 4 per wave), so every wave issues five pixel passes per clip like the block kernel does;
//   - a clip of raw data is 5 z2 float4 + 2 routed float4 + 2 index words = 30 registers (45 before); every staging address, halo offset
//     and window number is a per-thread constant computed once, and the tile -> (row, column) map divides by a constant;
//   - the BatchNorm coefficients are derived as before (bn_bwd_k_from_acc, block 0 leaves dgamma / dbeta / k2 / k3 and clears the other
//     parity's accumulator set), then parked in LDS and read back while staging, as kws_conv2_wgrad_fast.h does;
//   - in the product phase the fragments of a tap are read two taps in front of their products, into a ring that runs on into the wave's
//     next tile: cycle stamps showed the phase at twice its matrix time, each tap waiting an LDS round trip for fragments requested
//     one tap (96 matrix cycles) earlier.  The product is taken transposed (weights as the A operand), so that a lane holds four
//     channels of one pixel and a tile is stored with one 16-byte store per lane.
// One clip of raw data is in flight, as in the block kernel: a second one in registers and one landing in LDS by LDS-direct loads were
// both measured and were no faster (the loads are not what the loop waits for).
// The LDS plane layout ([plane][channel quarter][halo pixel][8 bf16], zero halo), the fragment reads, the weight fragments in registers,
// the tile rotation over the four waves and the arithmetic per element (dz2 expression and its operand order, split_bf16, the six products
// of mfma_bf16x6 in its order, the taps in (kh, kw) order in one accumulator per tile) are the block kernel's as written in the source.
// da1 is nevertheless NOT bit-equal to the block kernel's: the tensors it feeds sit 3.2e-6 .. 9.8e-6 from the exact-fp32 mode where the block
// kernel's sit 3.3e-6 .. 9.7e-6 (tests/test_conv2_dgrad_fast_gpu.py).  Every build of this kernel gave the same figures, with the product
// transposed or not, so the difference is taken to lie in how the compiler contracts and packs the dz2 expression (v_pk_fma_f32 here,
// v_fma_f32 there); that was read from the listings, not shown on a build with the contraction pinned.  Chosen by plan_cnn
// (dgrad2_fast); every other geometry, deterministic mode, a captured step and the fp32 mode keep the block kernel.
#pragma once
#include "kws_cnn_shape.h"   // kW2fH x kW2fW, the map the kernel is instantiated for: plan_cnn reads it

namespace kws {

template <int H, int W>
struct Conv2DgradFast {
    static constexpr int CR = 32, CO = 16, F4 = CR / 4, HP = H + 2, WP = W + 2, HW = H * W;
    static constexpr int NPIX = (HP * WP + 15) & ~15, NTILE = (HW + 15) / 16;   // rounded: the clamped rows of the last tile read inside the plane
    static constexpr int QUARTER = NPIX * 16, PLANE = 4 * QUARTER, BYTES = 3 * PLANE;   // bytes
    static constexpr int HPL = H / 2, WPL = W / 2, NWIN = HPL * WPL;
    static constexpr int WIN1 = 256 / F4;                          // windows staged one unit per thread
    static constexpr int LEFT = (NWIN - WIN1) * 4;                 // pixels of the windows behind them ...
    static constexpr int SLOTS = LEFT + (H - 2 * HPL) * W;         // ... and of the rows below the last window: one pixel per 8 lanes
    static constexpr int SPW = (SLOTS + 3) / 4;                    // pixel slots per wave
    static_assert(W % 2 == 0, "every column lies in a pool window");
    static_assert(NWIN >= WIN1 && SPW * F4 <= 64, "one window unit per thread, then at most one pixel per thread");
    static_assert(BYTES % 16 == 0 && BYTES <= 64 * 1024, "the planes fit the default dynamic LDS limit");
};

template <int H, int W>
__global__ __launch_bounds__(256, 2) void conv2_dgrad_fast_kernel(const float *__restrict__ wgt, float *__restrict__ dx, int B, BnBwdArgs bn)
{
    using G = Conv2DgradFast<H, W>;
    constexpr int CR = G::CR, CO = G::CO, F4 = G::F4, WP = G::WP, HW = G::HW, NTILE = G::NTILE, WPL = G::WPL, NWIN = G::NWIN;
    constexpr int QUARTER = G::QUARTER, PLANE = G::PLANE;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctile[];   // [3 planes][4 quarters][(H+2)(W+2)][8 bf16], zero halo
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, lq = lane >> 4;
    for (int i = threadIdx.x; i < G::BYTES / 16; i += 256) reinterpret_cast<f32x4 *>(ctile)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    bf16x8 wf[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wgt + (t * CO + li) * CR + 8 * lq);
        const f32x4 w1 = *reinterpret_cast<const f32x4 *>(wgt + (t * CO + li) * CR + 8 * lq + 4);
        bf16x4 h0, m0, l0, h1, m1, l1;
        split_bf16(w0, h0, m0, l0);
        split_bf16(w1, h1, m1, l1);
        wf[t][0] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        wf[t][1] = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
        wf[t][2] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }

    // BatchNorm coefficients of the 4 channels of every float4 a thread stages (c4 = threadIdx.x % 8 in both rounds): derived as in the block
    // kernel, then kept in LDS ([gi | mean | inv | k2 | k3][CR]) and read back while staging, so that they hold no registers during the products
    __shared__ __attribute__((aligned(16))) float coef[5][CR];
    const int c4 = threadIdx.x & (F4 - 1);
    {
        f32x4 gi, mean, inv;
        float k2[4], k3[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            inv[e] = bn.inv[c]; gi[e] = bn.gamma[c] * inv[e]; mean[e] = bn.mean[c];
        }
        bn_bwd_k_from_acc(bn, CR, c4, bn.dgamma && blockIdx.x == 0, k2, k3);
        if (bn.acc_clear_set && blockIdx.x == 0) acc_clear(bn.acc_clear_set, threadIdx.x, 256);
        if (threadIdx.x < F4) {
            *reinterpret_cast<f32x4 *>(&coef[0][4 * c4]) = gi;
            *reinterpret_cast<f32x4 *>(&coef[1][4 * c4]) = mean;
            *reinterpret_cast<f32x4 *>(&coef[2][4 * c4]) = inv;
            *reinterpret_cast<f32x4 *>(&coef[3][4 * c4]) = (f32x4){k2[0], k2[1], k2[2], k2[3]};
            *reinterpret_cast<f32x4 *>(&coef[4][4 * c4]) = (f32x4){k3[0], k3[1], k3[2], k3[3]};
        }
    }                                                             // the clip loop's first barrier orders these stores in front of their reads

    // staging tables, computed once.  Round 1: window threadIdx.x / 8, its four pixels at (2 wy + dy, 2 wx + dx): z2 float4 zo1 + 8 (W dy + dx),
    // LDS byte d1 + 16 (WP dy + dx), routed gradient and index word threadIdx.x.  Round 2: pixel slot SPW wave + lane / 8 -- a pixel of the
    // windows past WIN1 or of a row below the last window; d2 < 0: the thread has none (its loads read element 0 and are dropped)
    const int wy = (int)(threadIdx.x >> 3) / WPL, wx = (int)(threadIdx.x >> 3) % WPL;
    const int lds_c = (c4 >> 1) * QUARTER + (c4 & 1) * 8;
    const int zo1 = (2 * wy * W + 2 * wx) * F4 + c4;
    const int d1 = ((2 * wy + 1) * WP + 2 * wx + 1) * 16 + lds_c;
    int zo2 = 0, d2 = -1, q2 = 0, ce2 = 0x100;                     // ce2 = 0x100: no byte of the index word matches, g = 0
    {
        const int sl = wave * G::SPW + (lane >> 3);
        if (lane < G::SPW * F4 && sl < G::SLOTS) {
            int y, x;
            if (sl < G::LEFT) {
                const int win = G::WIN1 + sl / 4, e = sl % 4;
                y = 2 * (win / WPL) + (e >> 1); x = 2 * (win % WPL) + (e & 1);
                q2 = win * F4 + c4; ce2 = e;
            } else {
                y = 2 * G::HPL + (sl - G::LEFT) / W; x = (sl - G::LEFT) % W;
            }
            zo2 = (y * W + x) * F4 + c4;
            d2 = ((y + 1) * WP + x + 1) * 16 + lds_c;
        }
    }

    struct Raw { f32x4 z[5], g[2]; unsigned a[2]; };               // a clip's raw data: 30 registers
    auto prefetch = [&](int b, Raw &r) {                            // raw loads only, all in bounds: the selects happen when the clip is staged
        const f32x4 *zs = reinterpret_cast<const f32x4 *>(bn.z) + (long)b * HW * F4;
        const f32x4 *gws = reinterpret_cast<const f32x4 *>(bn.gw) + (long)b * NWIN * F4;
        const unsigned *ars = reinterpret_cast<const unsigned *>(bn.arg) + (long)b * NWIN * F4;
        r.g[0] = gws[threadIdx.x];
        r.a[0] = ars[threadIdx.x];
#pragma unroll
        for (int e = 0; e < 4; ++e) r.z[e] = zs[zo1 + ((e >> 1) * W + (e & 1)) * F4];
        r.g[1] = gws[q2];
        r.a[1] = ars[q2];
        r.z[4] = zs[zo2];
    };
    auto put = [&](int d, f32x4 v) {
        bf16x4 h, m, l;
        split_bf16(v, h, m, l);
        *reinterpret_cast<bf16x4 *>(ctile + d) = h;
        *reinterpret_cast<bf16x4 *>(ctile + d + PLANE) = m;
        *reinterpret_cast<bf16x4 *>(ctile + d + 2 * PLANE) = l;
    };
    auto stage = [&](const Raw &r) {
        const f32x4 gi = *reinterpret_cast<const f32x4 *>(&coef[0][4 * c4]), mean = *reinterpret_cast<const f32x4 *>(&coef[1][4 * c4]),
                    inv = *reinterpret_cast<const f32x4 *>(&coef[2][4 * c4]), k2 = *reinterpret_cast<const f32x4 *>(&coef[3][4 * c4]),
                    k3 = *reinterpret_cast<const f32x4 *>(&coef[4][4 * c4]);
        // g of an element from its window's routed value (the element the window's maximum came from takes it), then BatchNorm backward
        auto dz2 = [&](f32x4 gw, unsigned aw, int ce, f32x4 zv) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = (int)((aw >> (8 * e)) & 0xFFu) == ce ? gw[e] : 0.f;
                v[e] = gi[e] * (g - k2[e] - (zv[e] - mean[e]) * inv[e] * k3[e]);
            }
            return v;
        };
#pragma unroll
        for (int e = 0; e < 4; ++e) put(d1 + ((e >> 1) * WP + (e & 1)) * 16, dz2(r.g[0], r.a[0], e, r.z[e]));
        if (d2 >= 0) put(d2, dz2(r.g[1], r.a[1], ce2, r.z[4]));
    };
    // Products of the tiles t0, t0 + 4, ...: the fragments of a tap (one ds_read_b128 per plane) are read AHEAD taps in front of their
    // products, into a ring of AHEAD + 1 fragment sets, and the ring runs on into the next tile, so the one accumulator chain of a tile
    // does not wait an LDS round trip per tap (left to itself the compiler reads one tap ahead, 96 matrix cycles for a loaded LDS).
    // The product is taken transposed -- weights as the A operand, dz as B; the two fragment shapes are the same registers -- so that
    // a lane ends up with channels 4 lq .. 4 lq + 3 of pixel li: one 16-byte store per tile and lane instead of four scattered words.
    // Terms and their order are mfma_bf16x6's.
    constexpr int AHEAD = 2, RING = AHEAD + 1;
    static_assert(9 % RING == 0, "the ring position of tap 0 is the same in every tile");
    auto products = [&](int b, int t0) {
        auto origin = [&](int t) {                                 // halo pixel of this lane's row of tile t, tap (0, 0)
            const int p = 16 * t + li, pc = p < HW ? p : HW - 1;  // clamped: extra rows are not stored
            const int ih = pc / W, iw = pc - ih * W;               // W is a constant: a multiplication
            // source pixel of tap (kh, kw) in halo coordinates: (ih + 1 - kh + 1, iw + 1 - kw + 1)
            return ctile + lq * QUARTER + ((ih + 2) * WP + iw + 2) * 16;
        };
        bf16x8 a[RING][3];
        auto read = [&](const unsigned char *a0, int tap, bf16x8 (&f)[3]) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) f[pl] = *reinterpret_cast<const bf16x8 *>(a0 - ((tap / 3) * WP + tap % 3) * 16 + pl * PLANE);
        };
        const unsigned char *a0 = origin(t0);
#pragma unroll
        for (int tap = 0; tap < AHEAD; ++tap) read(a0, tap, a[tap % RING]);
        for (int t = t0; t < NTILE; t += 4) {
            const unsigned char *an = origin(t + 4 < NTILE ? t + 4 : t);   // last tile: the reads past it repeat its first taps and are dropped
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                if (tap + AHEAD < 9) read(a0, tap + AHEAD, a[(tap + AHEAD) % RING]);
                else read(an, tap + AHEAD - 9, a[(tap + AHEAD) % RING]);
                constexpr int pa[6] = {1, 2, 0, 1, 0, 0}, pb[6] = {1, 0, 2, 0, 1, 0};   // mfma_bf16x6(dz, w): small terms first
#pragma unroll
                for (int i = 0; i < 6; ++i) acc = mfma_bf16(wf[tap][pb[i]], a[tap % RING][pa[i]], acc);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int po = 16 * t + li;
            if (po < HW) *reinterpret_cast<f32x4 *>(dx + ((long)b * HW + po) * CO + 4 * lq) = acc;
            a0 = an;
        }
    };

    // the clip loop: barrier, stage the clip whose raw data has landed, barrier, request the next clip's raw data into the registers just
    // emptied, products.  The tile a wave starts with rotates from clip to clip, so every SIMD sees the same load over time.
    const int stride = gridDim.x;
    int rot = wave;
    Raw r;
    if ((int)blockIdx.x < B) prefetch(blockIdx.x, r);
    for (int b = blockIdx.x; b < B; b += stride, ++rot) {
        __syncthreads();                                          // previous clip's reads are done
        stage(r);
        __syncthreads();
        if (b + stride < B) prefetch(b + stride, r);              // in flight under this clip's products
        products(b, rot & 3);
    }
}

}  // namespace kws
