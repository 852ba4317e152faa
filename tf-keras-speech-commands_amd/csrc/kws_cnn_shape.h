// csrc/kws_cnn_shape.h -- shape and launch rules of simple_cnn / simple_cnn_lite (host only, free of HIP).
//
// Everything here is plain integer arithmetic: the map sizes of the four stages, TF 'SAME' padding, the convolution geometries, and how
// a launch is cut into blocks (the row split of the channel reductions, the stride-parity classes and MW of the data gradient, the
// one-resident-round grids of the weight gradients, the layer-1 and conv2 clip grids).  The launchers in kws_model.hip query the device
// (compute units, resident blocks of a kernel), call the rule and launch; plan_cnn (kws_cnn_plan.h) reads the shape constants below.
// The file includes standard headers and include/kws.h only, so a plain C++ compiler builds it: tests/host/cnn_shape_main.cpp answers
// queries about every rule and tests/test_cnn_shape_host.py holds the answers to the tests' Python restatements, without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kws.h"

namespace kws {

// ---- shape constants that plan_cnn reads; each names the kernel header that is built for it --------------------------------
constexpr int kStatStride = 1024;      // max blocks of a channel reduction; partial[(which*C + c)*kStatStride + blk]
                                       // (kws_layers.h: the reductions and their finalize kernels)
constexpr int kMaxStatBlocks = kStatStride;

// kws_infer_fused.h (the one-kernel inference tail) and kws_conv_group.h (the clip-group kernels of conv3 / conv4)
constexpr int kFuClips = 16;                      // clips per block = MFMA rows
constexpr int kFuH2 = 7, kFuW2 = 5;               // a2: input of conv3
constexpr int kFuH3 = 4, kFuW3 = 3;               // conv3 output (stride 2, 'same': pad 1 before on both axes)
constexpr int kFuH4 = 2, kFuW4 = 1;               // conv4 output 4 x 3 x 128, pooled 2 x 1 x 128
constexpr int kFuHeadCols = 48;                   // classes padded to three column tiles
// kws_conv_group.h (conv3_group_fwd_kernel with the pool of layer 2 fused)
constexpr int kGrH1 = 2 * kFuH2 + 1, kGrW1 = 2 * kFuW2;                         // conv2's map: 15 x 10 (the last row falls out of the 'valid' pooling)

// kws_layer1.h (the MFMA, wave-per-clip forms of layer 1)
constexpr int kL1MaxTiles = 40;      // tiles (4 pool windows each) per clip
constexpr int kL1Stage = 12;         // staged elements per lane: (H+2)(W+2) <= 64 * 12

// kws_dense_head.h (dense_head_fused_kernel)
constexpr int kDhK = 128;            // Dense units
// kDhWaves waves per block of 16 samples: every phase below is a chain of dependent LDS / L2 round trips with little work per wave, and
// the kernel shares its CU with the next batch's featurizer (twelve vector-ALU-bound waves) -- eight waves halve the serial work of a
// wave in the Dense product, the data gradient and the dW2 tiles against four (four waves: 0.037 ms alone, 0.115 under the featurizer).
constexpr int kDhWaves = 8;

// kws_conv2_wgrad_fast.h (conv2_wgrad_fast_kernel)
constexpr int kW2fH = 15, kW2fW = 10;                              // the map the kernel is instantiated for (kws_model.hip)

// ---- sizes -----------------------------------------------------------------------------------------------------------------
struct CnnDims { int H0, W0, H1, W1, H2, W2, H3, W3, H4, W4, flat; };

inline int64_t al4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_for(long n, int per) { return (unsigned)((n + per - 1) / per); }

inline int same_out(int n, int s) { return (n + s - 1) / s; }
inline int same_pad_before(int n, int k, int s)
{
    const int out = same_out(n, s), total = std::max((out - 1) * s + k - n, 0);
    return total / 2;   // TF 'SAME': the extra element goes to the end
}

// the maps of either CNN on an (n_features x feature_size) input; H4 < 1 or W4 < 1: the input is too small
inline CnnDims cnn_dims(int n_features, int feature_size)
{
    CnnDims d;
    d.H0 = n_features; d.W0 = feature_size;
    d.H1 = d.H0 / 2; d.W1 = d.W0 / 2;                 // MaxPooling2D(): 2x2, stride 2, 'valid'
    d.H2 = d.H1 / 2; d.W2 = d.W1 / 2;
    d.H3 = same_out(d.H2, 2); d.W3 = same_out(d.W2, 2);
    d.H4 = d.H3 / 2; d.W4 = d.W3 / 2;
    d.flat = d.H4 * d.W4 * 128;
    return d;
}

constexpr int kCh[5] = {1, 16, 32, 64, 128};

// Stage l = 0 .. 3 of either CNN: a 3x3 'same' convolution (a SeparableConv2D in simple_cnn_lite) from a (Hi x Wi x Cin) map to
// (Ho x Wo x Cout), then BatchNorm -> ReLU6 and, where pooled, a 2x2 max-pool.  relu: simple_cnn_lite's pointwise output carries
// activation='relu' (cnn.py:113,122)
struct CnnStage { int Hi, Wi, Ho, Wo, stride, Cin, Cout; bool pooled, relu; };
inline CnnStage cnn_stage(const CnnDims &d, int l)
{
    const int Hi[4] = {d.H0, d.H1, d.H2, d.H3}, Wi[4] = {d.W0, d.W1, d.W2, d.W3};
    const int stride = l == 2 ? 2 : 1;
    return CnnStage{Hi[l], Wi[l], same_out(Hi[l], stride), same_out(Wi[l], stride), stride, kCh[l], kCh[l + 1], l != 2, l >= 2};
}

// ---- convolution geometries (the kernels of kws_conv.h take them by value) ---------------------------------------------------
struct ConvGeom {
    int B, H, W, Ho, Wo;   // input and output spatial sizes (NHWC)
    int stride, pt, pl;    // TF 'SAME': pad_top / pad_left (the extra pad, if any, is bottom/right)
    int KH, KW;
    // conv_bf16_kernel only: rows in pixel-major order (row q = pixel q / B of clip q % B instead of clip-major), see there
    int pmajor = 0;
};

inline ConvGeom geom3x3(int B, int H, int W, int stride)
{
    ConvGeom g;
    g.B = B; g.H = H; g.W = W; g.stride = stride; g.KH = 3; g.KW = 3;
    g.Ho = same_out(H, stride); g.Wo = same_out(W, stride);
    g.pt = same_pad_before(H, 3, stride); g.pl = same_pad_before(W, 3, stride);
    return g;
}
inline ConvGeom geom1x1(int B, int H, int W)
{
    ConvGeom g;
    g.B = B; g.H = H; g.W = W; g.Ho = H; g.Wo = W; g.stride = 1; g.pt = 0; g.pl = 0; g.KH = 1; g.KW = 1;
    return g;
}
// Dense(128, use_bias=True) + ReLU6 as a (H4 x W4) 'valid' convolution over the pooled map (Flatten is h,w,c)
inline ConvGeom dense_geom(const CnnDims &d, int B)
{
    ConvGeom g;
    g.B = B; g.H = d.H4; g.W = d.W4; g.Ho = 1; g.Wo = 1; g.stride = 1; g.pt = 0; g.pl = 0; g.KH = d.H4; g.KW = d.W4;
    return g;
}

// ---- channel reductions ------------------------------------------------------------------------------------------------------
// rows-per-block and grid for the (M x C) channel reductions
inline void stat_grid(long M, int C, int &nblk, int &rows)
{
    const int R = 256 / C;
    long want = (M + (long)R * 8 - 1) / ((long)R * 8);
    nblk = (int)std::min<long>(kMaxStatBlocks, std::max<long>(1, want));
    rows = (int)((M + nblk - 1) / nblk);
    nblk = (int)((M + rows - 1) / rows);
}

// ---- the split-precision GEMM kernels (kws_conv.h: conv_bf16_kernel) -----------------------------------------------------------
// rows per block = 32 * RT: 96 for conv4's forward (8 column tiles: the larger tile halves the LDS reads per MFMA), 64
// elsewhere (3 resident blocks per CU overlap their staging and MFMA phases better; measured per kernel at B = 4096)
constexpr int conv_bf16_rt(bool fwd, int CR, int CO) { return (fwd && CO == 128 && CR == 64) ? 3 : 2; }
// small maps with 'same' padding: pixel-major rows let a block skip the taps that are padding for its position (kws_conv.h)
inline int conv_bf16_pmajor(const ConvGeom &g, bool fwd)
{
    const int P = fwd ? g.Ho * g.Wo : g.H * g.W;
    return (g.KH == 3 && g.KW == 3 && P > 1 && P <= 16) ? 1 : 0;
}

// ---- data gradient (kws_conv.h: conv_dgrad_direct_kernel) ------------------------------------------------------------------------
struct DgradClass { int cy, cx, ny, nx; };   // rows of the class: ih = stride*a + cy (a < ny), iw = stride*b + cx (b < nx)
struct DgradClasses { DgradClass c[4]; };     // one launch covers every class: blockIdx.y selects it (blocks past a class's rows exit)

// ONE launch over every stride-parity class of the input pixels (blockIdx.y = class).  MW (16-row tiles per wave) is picked so that the
// waves divide evenly over the SIMDs: every SIMD's matrix pipe then runs ceil(waves / SIMDs) * MW tile-times, and the smallest such
// product wins (ties: the larger MW reuses weights more).
struct DgradPlan { DgradClasses cls; int ncls; long max_rows; int mw; };
enum { DGRAD_OK = 0, DGRAD_KERNEL_TOO_LARGE = 1, DGRAD_STRIDE = 2 };    // more than 8 * stride taps per axis (the tap masks); a stride above 2
inline int dgrad_plan(const ConvGeom &g, long simds, DgradPlan &p)
{
    if (g.KH > 8 * g.stride || g.KW > 8 * g.stride) return DGRAD_KERNEL_TOO_LARGE;
    DgradClasses &cls = p.cls;
    int ncls = 0;
    long rows[4] = {0, 0, 0, 0}, max_rows = 0;
    for (int cy = 0; cy < g.stride && cy < 2; ++cy)
        for (int cx = 0; cx < g.stride && cx < 2; ++cx) {
            DgradClass c{cy, cx, (g.H - cy + g.stride - 1) / g.stride, (g.W - cx + g.stride - 1) / g.stride};
            if (c.ny <= 0 || c.nx <= 0) continue;
            rows[ncls] = (long)g.B * c.ny * c.nx;
            max_rows = std::max(max_rows, rows[ncls]);
            cls.c[ncls++] = c;
        }
    for (int i = ncls; i < 4; ++i) cls.c[i] = DgradClass{0, 0, 0, 0};
    if (g.stride > 2) return DGRAD_STRIDE;
    int best = 4;
    long best_cost = -1;
    for (int mw = 4; mw >= 1; --mw) {
        long waves = 0;
        for (int i = 0; i < ncls; ++i) waves += ((rows[i] + 15) / 16 + mw - 1) / mw;
        const long cost = ((waves + simds - 1) / simds) * mw;
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = mw; }
    }
    p.ncls = ncls; p.max_rows = max_rows; p.mw = best;
    return DGRAD_OK;
}

// ---- weight gradients ----------------------------------------------------------------------------------------------------------
// conv_wgrad_direct_kernel: `steps` 4-pixel MFMA k-steps over gx blocks along the pixel axis (gy along the tap groups), spw steps per
// wave.  The grid is sized so that all blocks are resident at once (ONE round): with more blocks than slots the
// last round runs on a fraction of the chip (measured on conv4: 990 blocks on 768 slots left the CUs idle 43 % of the time).
// resident = compute units * resident blocks per unit
struct WgradRound { long gx; int spw; };
inline WgradRound wgrad_round(long steps, int gy, long resident, bool deterministic)
{
    // deterministic: ONE block along the pixel axis, so every output element receives a single add onto the cleared buffer
    const long slots = deterministic ? 1 : std::max<long>(1, resident / gy); // blocks along x that fit at once
    // >= 8 steps per wave so the end-of-block tile reduction amortises
    const long gx_want = std::max<long>(1, std::min<long>(slots, (steps + 4 * 8 - 1) / (4 * 8)));
    const int spw = (int)((steps + 4 * gx_want - 1) / (4 * gx_want));
    const long gx = (steps + 4L * spw - 1) / (4L * spw);
    return WgradRound{gx, spw};
}

// conv_wgrad_bf16_kernel: grid = (tap groups) * (pixel ranges), one resident round, the taps of a range on one XCD; cpb 32-pixel chunks
// per block
struct WgradBf16Round { long nranges; int cpb; };
inline WgradBf16Round wgrad_bf16_round(long nchunk, int ngroups, long resident, bool deterministic)
{
    // ranges: a multiple of 8 (one per XCD), at most one resident round, at least 4 chunks per block
    long nranges = std::max<long>(8, (resident / ngroups) / 8 * 8);
    nranges = std::min<long>(nranges, std::max<long>(8, (nchunk / 4 + 7) / 8 * 8));
    int cpb = (int)((nchunk + nranges - 1) / nranges);
    if (deterministic) { nranges = 8; cpb = (int)nchunk; }   // range 0 takes every chunk: a single add per output element
    return WgradBf16Round{nranges, cpb};
}

// The position-major form of conv_wgrad_bf16_kernel for output maps of at most 16 pixels (kws_conv.h describes the kernel's side)
struct WgradPm {
    unsigned long long pos[9];    // per tap: the output positions at which it reads inside the map, a nibble each
    int npos[9];                  // ... and how many they are
    int slot0[10];                // first slot of each tap within an XCD; slot0[taps] = slots per XCD (grid = 8 x that)
};

// The host side of the position-major form: the lists and the slot shares for one launch (tests/wgrad_pmajor_cases.py restates it).
//   lists   tap (kh, kw) keeps the output positions p = oy Wo + ox at which it reads inside the map (0 <= oy stride + kh - pt < H and
//           0 <= ox stride + kw - pl < W); its weight w is their number
//   slots   S slots per XCD: enough for `min_chunks` chunks per block on average, at least one per tap that has positions and at most
//           max_slots (one resident round); a tap starts from floor(S w / sum w) slots (at least 1), then slots go one by one to the
//           tap with the most positions per slot (lowest index on ties) -- or, while there are too many, leave the tap with the
//           fewest (highest index on ties) -- until they add up to S
// false: a map of more than 16 pixels, more than nine taps, or fewer slots than taps
inline bool wgrad_pm_plan(const ConvGeom &g, int max_slots, int min_chunks, WgradPm &pm)
{
    const int P = g.Ho * g.Wo, ntaps = g.KH * g.KW;
    if (P < 1 || P > 16 || ntaps < 1 || ntaps > 9) return false;
    long w[9], wsum = 0;
    int live = 0;
    for (int tap = 0; tap < ntaps; ++tap) {
        const int kh = tap / g.KW, kw = tap % g.KW;
        pm.pos[tap] = 0ull; pm.npos[tap] = 0;
        for (int p = 0; p < P; ++p) {
            const int sy = (p / g.Wo) * g.stride + kh - g.pt, sx = (p % g.Wo) * g.stride + kw - g.pl;
            if (sy < 0 || sy >= g.H || sx < 0 || sx >= g.W) continue;
            pm.pos[tap] |= (unsigned long long)p << (4 * pm.npos[tap]);
            ++pm.npos[tap];
        }
        w[tap] = pm.npos[tap]; wsum += w[tap]; live += w[tap] > 0;
    }
    if (live < 1 || max_slots < live) return false;
    const long nclip = ((long)g.B + 31) / 32, want = (wsum * nclip + 8L * min_chunks - 1) / (8L * min_chunks);
    const int S = (int)(want < live ? live : want > max_slots ? max_slots : want);
    int s[9], total = 0;
    for (int tap = 0; tap < ntaps; ++tap) {
        s[tap] = w[tap] ? (int)((long)S * w[tap] / wsum) : 0;
        if (w[tap] && s[tap] < 1) s[tap] = 1;
        total += s[tap];
    }
    for (; total < S; ++total) {
        int best = -1;
        for (int tap = 0; tap < ntaps; ++tap)
            if (w[tap] && (best < 0 || w[tap] * s[best] > w[best] * s[tap])) best = tap;
        ++s[best];
    }
    for (; total > S; --total) {
        int best = -1;
        for (int tap = 0; tap < ntaps; ++tap)
            if (s[tap] > 1 && (best < 0 || w[tap] * s[best] <= w[best] * s[tap])) best = tap;
        --s[best];
    }
    pm.slot0[0] = 0;
    for (int tap = 0; tap < ntaps; ++tap) pm.slot0[tap + 1] = pm.slot0[tap] + s[tap];
    for (int tap = ntaps + 1; tap < 10; ++tap) pm.slot0[tap] = pm.slot0[ntaps];
    return true;
}

// ---- clip grids ------------------------------------------------------------------------------------------------------------------
// the layer-1 kernels, forward and backward (kws_layer1.h)
struct L1Grid {
    int cpb, nb;        // clips per block and blocks of the block-per-clip forms
    int cpw, nbm;       // clips per wave and blocks of the MFMA, wave-per-clip forms
};
inline L1Grid l1_grid(int B)
{
    L1Grid g;
    g.cpb = std::max(1, (B + kMaxStatBlocks - 1) / kMaxStatBlocks); g.nb = (B + g.cpb - 1) / g.cpb;
    g.cpw = std::max(1, (B + 4 * kMaxStatBlocks - 1) / (4 * kMaxStatBlocks)); g.nbm = (B + 4 * g.cpw - 1) / (4 * g.cpw);
    return g;
}

// persistent grids of conv2's clip-resident kernels: at most max_blocks (the LDS-limited residency), with an equal share of clips each
inline unsigned even_grid(int B, int max_blocks) { const int cpb = (B + max_blocks - 1) / max_blocks; return (unsigned)((B + cpb - 1) / cpb); }

// simple_cnn_lite's front inference kernel (kws_lite.h), one wave per clip and sm bytes of LDS per wave: up to 8 waves per compute unit
// within 160 KB; beyond them a wave takes cpw clips
struct LiteFrontGrid { int cpw, nblk; };
inline LiteFrontGrid lite_front_grid(int B, int cus, size_t sm)
{
    const int waves = cus * std::max(1, std::min(8, (int)(160 * 1024 / sm)));
    const int cpw = std::max(1, (B + waves - 1) / waves), nblk = (B + cpw - 1) / cpw;
    return LiteFrontGrid{cpw, nblk};
}

// ---- the head ------------------------------------------------------------------------------------------------------------------
// whether the MFMA form of the head's backward kernel applies (kws_layers.h: head_bwd_mfma_kernel): Dense(C) on a K-wide feature vector
inline bool head_bwd_fuses(int K, int C) { return K % 16 == 0 && K <= 128 && C <= 48; }

}  // namespace kws
