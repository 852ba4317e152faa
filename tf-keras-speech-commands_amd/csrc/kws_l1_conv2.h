// csrc/kws_l1_conv2.h -- layer 1 (conv1 -> BatchNorm 1 from the feature moments -> ReLU6 -> 2x2 max) and conv2's forward with its
// BatchNorm-2 sums in ONE clip-resident train kernel (split precision, compile-time map, accumulator-form statistics).
//
// The two-kernel path (kws_layer1_moments.h: l1m_act_pool_moments_kernel<true>, then kws_conv.h: conv_fwd_clip_bf16_kernel<true>) writes
// a1 and reads it straight back, runs layer 1 one wave per clip with nothing beside it, and drains / fills the chip between the two.
// Here a block owns whole clips (b = blockIdx.x + k * nclip_blocks, the conv2 kernel's clip order) and keeps everything of a clip
// between the feature map and z2 in LDS:
//   - the clip's haloed map is staged once per block; the next clip's features (HW floats, < 3 per thread) are fetched into registers
//     while the current clip is computed;
//   - the four waves share the clip's layer-1 tiles: L1Runs<H, W>::RR = 4, so wave w takes window row w of every quadrant run of
//     l1f_forward_clips (same mfma16 chains, same tap grouping, same fmaf / max / relu6f), and the pooled value goes to global a1
//     (conv2's weight gradient still reads it) and, split into h / m / l with split_bf16, straight into conv2's bf16 planes (the
//     [plane][channel half][halo pixel][8] layout conv_fwd_clip_bf16_kernel's stage() writes);
//   - behind one barrier, conv2 runs as conv_fwd_clip_bf16_kernel<true> does: the same 5 x 3 weight fragments in registers, the same
//     mfma_bf16x6 k-steps, tile split, z2 stores and per-lane BatchNorm sums, added to the same accumulator set (acc_add).
// The same helpers in the same order: a1 and z2 are bit-identical to the two-kernel path, and every lane's BatchNorm-2 sums see the
// same values in the same order (tests/test_l1_conv2_fused_gpu.py).  Two barriers per clip: the map of clip b + 1 is staged into the
// (by then free) map tile between layer 1 and conv2 of clip b.  The kPrepBlocks extra blocks behind the clip blocks do what the
// layer-1 kernel's PREP blocks do (l1_prep_block).
#pragma once

namespace kws {

// LDS bytes of l1_conv2_fwd_bf16_kernel<H, W>: the bf16 planes of the pooled map, then the haloed feature map (L1Runs::TILE floats)
template <int H, int W>
struct L1Conv2Lds {
    static constexpr int H2 = H / 2, W2 = W / 2, WP2 = W2 + 2, NPIX = ((H2 + 2) * WP2 + 15) & ~15;
    static constexpr int PLANES = 6 * NPIX * 16, BYTES = PLANES + 4 * L1Runs<H, W>::TILE;
};

template <int H, int W>
__global__ __launch_bounds__(256, 4) void l1_conv2_fwd_bf16_kernel(const float *__restrict__ feat, const float *__restrict__ wk,
                                                                   const double *__restrict__ q, const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, float *__restrict__ moving_mean,
                                                                   float *__restrict__ moving_var, BnCoef k, float *__restrict__ a1,
                                                                   const float *__restrict__ wgt, float *__restrict__ z, double *__restrict__ acc_out,
                                                                   int B, int nclip_blocks, L1PrepArgs prep)
{
    using R = L1Runs<H, W>;
    using L = L1Conv2Lds<H, W>;
    constexpr int WP = R::WP, Wp = R::Wp, NWIN = R::NWIN, HW = R::HW, RL = R::RL, RR = R::RR;
    constexpr int CIN = 16, COUT = 32, W2 = L::W2, WP2 = L::WP2, HW2 = NWIN, NPIX = L::NPIX, NT2 = (HW2 + 15) / 16;
    constexpr int NFE = (HW + 255) / 256;                          // feature values per thread and clip
    static_assert(RR == 4 && Wp == W2, "one window row of every quadrant run per wave");
    if ((int)blockIdx.x >= nclip_blocks) { l1_prep_block(prep, blockIdx.x - nclip_blocks); return; }
    extern __shared__ __attribute__((aligned(16))) unsigned char ctile[];
    float *xs = reinterpret_cast<float *>(ctile + L::PLANES);
    __shared__ float s_sc[16], s_sh[16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, lq = lane >> 4;

    float pre[NFE];
    auto fetch = [&](long b) {
#pragma unroll
        for (int j = 0; j < NFE; ++j) {
            const int f = threadIdx.x + 256 * j;
            pre[j] = f < HW ? feat[b * HW + f] : 0.f;
        }
    };
    auto stage = [&]() {                                           // interior of the haloed map; the halo stays zero
#pragma unroll
        for (int j = 0; j < NFE; ++j) {
            const int f = threadIdx.x + 256 * j;
            if (f < HW) xs[(f / W + 1) * WP + f % W + 1] = pre[j];
        }
    };
    const int b0 = blockIdx.x;                                     // < B: nclip_blocks = min(B, ...)
    fetch(b0);
    l1_bn_prologue(q, wk, gamma, beta, moving_mean, moving_var, k, s_sc, s_sh);
    for (int i = threadIdx.x; i < L::BYTES / 4; i += 256) reinterpret_cast<unsigned *>(ctile)[i] = 0u;

    // layer 1: conv1 B fragments W[tap = 4j + lq][c = li] and the tap offsets, as l1f_forward_clips; A side = pixel (quadrant run
    // qa = li >> 2, element e = li & 3) of window row `wave` of that run
    float wb[3];
    const float *abase[3];
    {
        const int qa = li >> 2, e = li & 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int tap = 4 * j + lq, tc = tap < 9 ? tap : 8;
            wb[j] = tap < 9 ? wk[tap * 16 + li] : 0.f;
            abase[j] = xs + 2 * (RR * qa) * WP + (e >> 1) * WP + (e & 1) + (tc / 3) * WP + tc % 3 + wave * 2 * WP;
        }
    }
    // D side: lane (channel li, run lq) owns window row py = RR lq + wave of the pooled map (quadrant 3's fourth row lies past it)
    const int py = RR * lq + wave;
    const bool wrow = py < H / 2;
    const int a1off = (RL * lq + wave * Wp) * 16 + li;            // window RL lq + wave Wp of the clip, channel li
    unsigned char *pdst = ctile + (((li >> 3) * NPIX + (py + 1) * WP2 + 1) * 16 + (li & 7) * 2);

    // conv2: B fragments of k-step s, lane holds W[tap][8 (lq & 1) + j][16 nt + li], tap = 2 s + (lq >> 1) (conv_fwd_clip_bf16_kernel)
    const int nt = wave & 1, tpar = wave >> 1;
    bf16x8 wf[5][3];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int tap = 2 * st + (lq >> 1);
        f32x4 w0 = {0.f, 0.f, 0.f, 0.f}, w1 = {0.f, 0.f, 0.f, 0.f};
        if (tap < 9) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w0[j] = wgt[(tap * CIN + 8 * (lq & 1) + j) * COUT + 16 * nt + li];
                w1[j] = wgt[(tap * CIN + 8 * (lq & 1) + 4 + j) * COUT + 16 * nt + li];
            }
        }
        bf16x4 h0, m0, l0, h1, m1, l1;
        split_bf16(w0, h0, m0, l0);
        split_bf16(w1, h1, m1, l1);
        wf[st][0] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        wf[st][1] = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
        wf[st][2] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    int aoff[5];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int tap = 2 * st + (lq >> 1), tc = tap < 9 ? tap : 8;
        aoff[st] = (((lq & 1) * NPIX) + (tc / 3) * WP2 + tc % 3) * 16;
    }
    float ssum = 0.f, ssq = 0.f;

    __syncthreads();                                               // the LDS is zero, s_sc / s_sh are in place
    stage();
    if (b0 + nclip_blocks < B) fetch(b0 + nclip_blocks);
    const float sc = s_sc[li], sh = s_sh[li];
    __syncthreads();
    for (int b = b0; b < B; b += nclip_blocks) {
        // layer 1 of clip b: Wp tiles with immediate offsets, the next tile's product issued before this one is finished
        {
            float *out = a1 + (long)b * NWIN * 16 + a1off;
            auto zprod = [&](int c) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 3; ++j) acc = mfma16(abase[j][2 * c], wb[j], acc);
                return acc;
            };
            f32x4 zc = zprod(0);
#pragma unroll
            for (int c = 0; c < Wp; ++c) {
                const f32x4 zn = c + 1 < Wp ? zprod(c + 1) : zc;
                const float y0 = fmaf(zc[0], sc, sh), y1 = fmaf(zc[1], sc, sh), y2 = fmaf(zc[2], sc, sh), y3 = fmaf(zc[3], sc, sh);
                const float v = relu6f(fmaxf(fmaxf(y0, y1), fmaxf(y2, y3)));
                if (wrow) {
                    out[c * 16] = v;
                    bf16x4 h, m, l;
                    split_bf16((f32x4){v, 0.f, 0.f, 0.f}, h, m, l);
                    *reinterpret_cast<__bf16 *>(pdst + c * 16) = h[0];
                    *reinterpret_cast<__bf16 *>(pdst + c * 16 + 2 * NPIX * 16) = m[0];
                    *reinterpret_cast<__bf16 *>(pdst + c * 16 + 4 * NPIX * 16) = l[0];
                }
                zc = zn;
            }
        }
        __syncthreads();                                           // the planes of clip b are complete, the map tile is free
        if (b + nclip_blocks < B) {
            stage();
            if (b + 2 * nclip_blocks < B) fetch(b + 2 * nclip_blocks);
        }
        // conv2 of clip b: waves split (column tile nt, tile parity tpar)
        for (int t = tpar; t < NT2; t += 2) {
            const int p = 16 * t + li, pc = p < HW2 ? p : HW2 - 1;
            const int oh = pc / W2, ow = pc % W2;
            const unsigned char *ap = ctile + (oh * WP2 + ow) * 16;   // tap (0,0) of this pixel in halo coordinates
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 5; ++st) {
                bf16x8 a[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) a[pl] = *reinterpret_cast<const bf16x8 *>(ap + aoff[st] + pl * 2 * NPIX * 16);
                acc = mfma_bf16x6(a, wf[st], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int po = 16 * t + 4 * lq + r;
                if (po < HW2) {
                    const float v = acc[r];
                    z[((long)b * HW2 + po) * COUT + 16 * nt + li] = v;
                    ssum += v; ssq = fmaf(v, v, ssq);
                }
            }
        }
        __syncthreads();                                           // conv2 is done with the planes, clip b + 1's map is staged
    }
    // BatchNorm-2 sums as conv_fwd_clip_bf16_kernel<true>: over lq (xor 16, 32), then over the two waves of the column tile
    double *red = reinterpret_cast<double *>(ctile);             // [4 waves][2][16]
    double a = (double)ssum, sq = (double)ssq;
    a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
    sq += __shfl_xor(sq, 16, 64); sq += __shfl_xor(sq, 32, 64);
    if (lq == 0) { red[(wave * 2 + 0) * 16 + li] = a; red[(wave * 2 + 1) * 16 + li] = sq; }
    __syncthreads();
    if (threadIdx.x < 2 * COUT) {
        const int which = threadIdx.x / COUT, c = threadIdx.x % COUT, n = c / 16, l = c % 16;
        const double v = red[(n * 2 + which) * 16 + l] + red[((n + 2) * 2 + which) * 16 + l];
        acc_add(acc_out, 2 * COUT, threadIdx.x, v);
    }
}

}  // namespace kws
