// csrc/kws_featurize.hip -- fused waveform -> MFCC/BFCC featurizer for gfx950 (MI355X).
//
// Replaces common/data_utils.py:73-86 (audio_to_feature -> vectorize_raw -> sonopy.mfcc_spec,
// optional add_deltas) of the reference for a whole batch in one launch.
//
// Mapping (n_fft = 1024 path):
//   block  = one clip, kWaves wavefronts of 64 lanes;  wave w owns frames w, w+kWaves, ...
//   frame  = 1024 real samples -> 512-point complex FFT done entirely inside ONE wave:
//            each lane holds 8 complex points, three radix-8 passes (8x8x8) with two
//            transposes through a per-wave 4.5 KB LDS tile (padded 72/9 so every half-wave
//            ds_read/ds_write_b64 is bank-conflict free), then the real-FFT split,
//            |X|^2/n_fft, a SPARSE band gather for the filterbank (per-lane chunks of one
//            band's non-zero span; no dense GEMM), eps-clipped log, ortho DCT-II, c0 <- log energy.
//   HBM    : every sample is requested once per frame it belongs to (2x with hop = window/2);
//            the second touch is an L1/L2 hit issued by the same block, so DRAM traffic stays at
//            the algorithmic 4 B/sample in + 4 B/feature out.
#include <memory>
#include <type_traits>

#include "kws_common.h"
#include "kws_device.h"
#include "kws_augment.h"
#include "kws_featurize_tables.h"   // the host side: geometry, bank, chunk tables, twiddles, DCT, table arena

namespace kws {

constexpr int kWaves = 5;                 // wavefronts per clip (30 default frames -> 6 frames each)
constexpr int kThreads = kWaves * 64;
constexpr int kFftTile = 8 * 72;          // float2 elements per wave (padded 8 x 64 tile)
constexpr float kEps = 2.220446049250313e-16f;  // np.finfo(float).eps, common/bark_feature.py:77

struct FeatDev {
    int window_eff, hop, max_samples, n_frames, n_filt, n_out, feature_size, use_delta, nchunks, nnz;
    int chp, n_filt_pad;   // chunk length padded to a multiple of 4 (zero weights); n_filt rounded up to 4 (zero DCT rows)
    int tail_batch;        // frames whose band sums / DCT one wave evaluates together (lanes = frames x bands)
    int fpw, jpc;          // frames per wave job, jobs per clip (set per launch: launch_featurize)
    const int32_t *index;  // NULL, or B device ints: clip b is ROW index[b] of wav / valid_len (kws_featurize_gather; set per launch)
    float inv_nfft;
    const float2 *tw1;   // [7][64]  W_512^(lane*k1), k1 = 1..7
    const float2 *tw2;   // [7][8]   W_64^(l2*k2a),   k2a = 1..7
    const float2 *tws;   // [257]    W_1024^k
    const int4 *chunks;  // [64 lanes] {band, first bin read, chunk id, 0}: lane placement is bank-conflict free (host matching)
    const int *bcs;      // [n_filt+1] first chunk of each band
    const float *w;      // [64 lanes][chp] bank weights of the lane's window, zero outside its chunk (nnz = 64*chp)
    const float *dct;    // [n_filt_pad][n_out], ortho scaling folded in, zero rows past n_filt
    // generic path (n_fft != 1024): radix-2 twiddles and the bank as per-band spans
    int n_fft, log2n;
    const float2 *twg;   // [n_fft/2]  W_nfft^k
    const int *bfirst;   // [n_filt] first non-zero bin of each band
    const int *bwidth;   // [n_filt] span length
    const float *bw;     // [n_filt][n_bins] dense bank rows (float)
    // tuned kernel (kws_featurize_v3.h): lane-linear LDS stores; chunks over POSITIONS of the two power planes, weights x 2^-12
    int chp3, blocks_per_cu;
    const int4 *chunks3; // [64 lanes] {band, first position read (even), chunk id, 0}
    const int *bcs3;     // [n_filt+1]
    const float *w3;     // [64 lanes][chp3]
    const float2 *tw1s;  // [7][64]  W_512^(sigma(lane) A), sigma(lane) = 8 (lane & 7) + (lane >> 3)
    const float2 *tws3;  // [4][64]  W_1024^(lane + 64 i)
};

}  // namespace kws

struct kws_featurizer {
    kws_params params;
    kws_geometry geom;
    int bank_kind;
    std::vector<float> bank;  // dense host copy (n_filt x n_bins)
    kws::FeatDev dev;
    void *dmem;               // one device allocation holding every table
    size_t smem_bytes;
    int blocks_per_cu = 2;    // persistent blocks per CU of the tuned kernel (kws_featurizer_set_cu_share)
};

namespace kws {

__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

// forward 8-point DFT in registers, natural order in and out
__device__ __forceinline__ void dft8(float2 (&v)[8])
{
    const float h = 0.70710678118654752440f;
    float2 a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]);
    float2 a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
    float2 a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
    float2 a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
    float2 b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
    float2 b4 = cadd(a4, a6), b6 = csub(a4, a6), b5 = cadd(a5, a7), b7 = csub(a5, a7);
    float2 t1 = make_float2(h * (b5.x + b5.y), h * (b5.y - b5.x));    // b5 * (1 - i)/sqrt2
    float2 t2 = mul_mi(b6);                                           // b6 * (-i)
    float2 t3 = make_float2(h * (b7.y - b7.x), -h * (b7.x + b7.y));   // b7 * (-1 - i)/sqrt2
    v[0] = cadd(b0, b4); v[4] = csub(b0, b4);
    v[1] = cadd(b1, t1); v[5] = csub(b1, t1);
    v[2] = cadd(b2, t2); v[6] = csub(b2, t2);
    v[3] = cadd(b3, t3); v[7] = csub(b3, t3);
}

// all 64 lanes of a wave run in lockstep and the LDS serves one wave's DS ops in order, so a
// compiler-level fence is all an intra-wave LDS exchange needs
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(short v) { return (float)v * (1.0f / 32768.0f); }  // data_utils.py:21

template <typename WavT> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<short> { using type = short2; };

__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }

// Complex points J0..J0+3 of the frame at sample `base`: z[n] = x[2n] + i x[2n+1], n = lane + 64 j.  A frame that lies
// wholly inside the recorded samples (wave-uniform test) takes the branch-free path: one address, immediate offsets.
template <typename WavT, int J0>
__device__ __forceinline__ void load_half(float2 (&v)[4], const WavT *__restrict__ src, int base, int pad, int window_eff,
                                          bool vec_ok, int lane)
{
    using V2 = typename Vec2<WavT>::type;
    if (vec_ok && base >= pad && window_eff >= 1024) {
        const V2 *p2 = reinterpret_cast<const V2 *>(src + (base - pad)) + lane + 64 * J0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const V2 t = p2[64 * j];
            v[j] = make_float2(to_f32(t.x), to_f32(t.y));
        }
    } else if (vec_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s0 = 2 * (lane + 64 * (J0 + j)), p0 = base + s0;
            float2 val = make_float2(0.f, 0.f);
            if (s0 < window_eff && p0 >= pad) {
                const V2 t = *reinterpret_cast<const V2 *>(src + (p0 - pad));
                val = make_float2(to_f32(t.x), to_f32(t.y));
            }
            v[j] = val;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s0 = 2 * (lane + 64 * (J0 + j)), p0 = base + s0;
            float2 val = make_float2(0.f, 0.f);
            if (s0 < window_eff && p0 >= pad) val.x = to_f32(src[p0 - pad]);
            if (s0 + 1 < window_eff && p0 + 1 >= pad) val.y = to_f32(src[p0 + 1 - pad]);
            v[j] = val;
        }
    }
}

// One block per clip, each wave owns a run of consecutive frames.  The kernel is bound by instruction issue (about 900
// wave instructions per frame, 5 waves per SIMD), so the structure is chosen to cut instructions rather than bytes:
//   * consecutive frames overlap by half when hop = n_fft/2: the upper half of frame f is the lower half of frame f+1 and
//     stays in registers, so a frame costs 4 loads per lane, issued one frame ahead;
//   * the band sum, log and DCT run once per `tail_batch` frames with lane = (frame, band) / (frame, coefficient), which
//     keeps ~60 of 64 lanes busy instead of 20; results go straight to global memory (no staging unless use_delta);
//   * per-lane table entries (chunk start, band span) live in registers, not LDS.
// LDS per block stays under 40 KB for 4 blocks per CU.
template <typename WavT>
__global__ __launch_bounds__(kThreads, 5) void featurize_fft1024_kernel(const WavT *__restrict__ wav, int64_t stride,
                                                                      const int32_t *__restrict__ valid_len, int B,
                                                                      FeatDev c, float *__restrict__ feat)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    // the wave index is uniform: telling the compiler so keeps the frame loop, its counters and branches in scalar registers
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // A wave owns one JOB = c.fpw consecutive frames of one clip.  Without deltas the jobs of all clips are dealt to the
    // waves in order (job = blockIdx.x * kWaves + wave), so short clips -- a streaming step featurizes 2 frames per stream --
    // still fill every wave; at the default geometry (30 frames, 6 per job, 5 jobs per clip) this is block = clip.  With
    // deltas the block keeps one clip (its coefficients are staged in s_feat for the frame differences).
    const int job = c.use_delta ? (wave < c.jpc ? (int)blockIdx.x * c.jpc + wave : -1) : (int)blockIdx.x * kWaves + wave;
    const int b = job < 0 ? B : job / c.jpc;

    const int tb = c.tail_batch;
    float2 *s_fft = reinterpret_cast<float2 *>(smem) + wave * kFftTile;
    float *s_pw = reinterpret_cast<float *>(s_fft);                       // power spectrum aliases the FFT tile
    float *s_part = reinterpret_cast<float *>(smem + kWaves * kFftTile * 8) + wave * (tb * 64 + 64 + 4);   // [tb][64]
    float *s_mel = s_part + tb * 64;                                       // [tb][n_filt_pad] (<= 64)
    float *s_en = s_mel + 64;                                              // [tb] (<= 4)
    float *s_dct = reinterpret_cast<float *>(smem + kWaves * kFftTile * 8) + kWaves * (tb * 64 + 64 + 4);
    float *s_w = s_dct + round4(c.n_filt_pad * c.n_out);
    float2 *s_tw1 = reinterpret_cast<float2 *>(s_w + round4(c.nnz));      // [7][64]
    float2 *s_tw2 = s_tw1 + 7 * 64;                                        // [7][8]
    int *s_bcs = reinterpret_cast<int *>(s_tw2 + 7 * 8);                   // [n_filt + 1] first chunk of each band (<= 68 ints)
    float *s_feat = reinterpret_cast<float *>(s_bcs + 68);                 // [n_frames][n_out], only with use_delta

    for (int i = tid; i < c.n_filt_pad * c.n_out; i += kThreads) s_dct[i] = c.dct[i];
    for (int i = tid; i < c.nnz; i += kThreads) s_w[i] = c.w[i];
    for (int i = tid; i < 7 * 64; i += kThreads) s_tw1[i] = c.tw1[i];
    for (int i = tid; i < 7 * 8; i += kThreads) s_tw2[i] = c.tw2[i];
    for (int i = tid; i <= c.n_filt; i += kThreads) s_bcs[i] = c.bcs[i];
    s_mel[lane] = 0.f;                                                     // the zero padding past n_filt is read by the DCT
    __syncthreads();

    // clip geometry: keep the head, left-pad zeros (data_utils.py:77-80)
    const int bc = b < B ? b : 0;                                          // idle waves (no job) read clip 0's geometry and do nothing
    const int row = c.index ? c.index[bc] : bc;
    int len = valid_len ? valid_len[row] : (stride > c.max_samples ? c.max_samples : (int)stride);
    len = len < 0 ? 0 : len;
    if ((int64_t)len > stride) len = (int)stride;
    if (len > c.max_samples) len = c.max_samples;
    const int pad = c.max_samples - len;
    const WavT *src = wav + (int64_t)row * stride;
    const bool vec_ok = (((pad | c.hop | c.window_eff) & 1) == 0) &&
                        ((reinterpret_cast<uintptr_t>(src) & (2 * sizeof(WavT) - 1)) == 0);
    const bool reuse = 2 * c.hop == 1024 && c.window_eff == 1024;          // frame f+1 starts with frame f's upper half

    const int hi = lane >> 3, lo = lane & 7;
    // per-lane roles in the batched tail
    // gather: lane = one chunk of one band; its first bin and its chunk id (the slot of its partial sum) packed in one register
    const int chunk_pack = c.chunks[lane].y | (c.chunks[lane].z << 16);
    const float r_filt = 1.0f / (float)c.n_filt, r_out = 1.0f / (float)c.n_out;
    float *dst = feat + (int64_t)bc * c.n_frames * c.feature_size;

    const int f_beg = b < B ? (job - b * c.jpc) * c.fpw : c.n_frames;
    const int f_end = f_beg + c.fpw < c.n_frames ? f_beg + c.fpw : c.n_frames;

    float2 xl[4], xh[4];                // lower / upper half of the next frame to transform
    if (f_beg < f_end) {
        load_half<WavT, 0>(xl, src, f_beg * c.hop, pad, c.window_eff, vec_ok, lane);
        load_half<WavT, 4>(xh, src, f_beg * c.hop, pad, c.window_eff, vec_ok, lane);
    }
    int qi = 0;                          // frames waiting in this wave's tail batch
    for (int f = f_beg; f < f_end; ++f) {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = xl[j]; v[j + 4] = xh[j]; }
        if (f + 1 < f_end) {             // next frame's samples: their HBM latency hides under this frame's FFT
            if (reuse) {
#pragma unroll
                for (int j = 0; j < 4; ++j) xl[j] = xh[j];
            } else {
                load_half<WavT, 0>(xl, src, (f + 1) * c.hop, pad, c.window_eff, vec_ok, lane);
            }
            load_half<WavT, 4>(xh, src, (f + 1) * c.hop, pad, c.window_eff, vec_ok, lane);
        }

        // pass 1: DFT-8 over n1 (n = lane + 64 n1), twiddle W_512^(lane*k1)
        dft8(v);
#pragma unroll
        for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], s_tw1[(k - 1) * 64 + lane]);
        wave_sync();
#pragma unroll
        for (int k = 0; k < 8; ++k) s_fft[72 * k + lane] = v[k];
        wave_sync();
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s_fft[72 * hi + lo + 8 * j];

        // pass 2: lane = (k1, l2); DFT-8 over l1, twiddle W_64^(l2*k2a)
        dft8(v);
#pragma unroll
        for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], s_tw2[(k - 1) * 8 + lo]);
        wave_sync();
#pragma unroll
        for (int k = 0; k < 8; ++k) s_fft[72 * hi + 9 * k + lo] = v[k];
        wave_sync();
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s_fft[72 * hi + 9 * lo + j];

        // pass 3: lane = (k1, k2a); DFT-8 over l2 -> Z[k1 + 8 k2a + 64 k2b]
        dft8(v);
        wave_sync();
#pragma unroll
        for (int r = 0; r < 8; ++r) {       // natural order k = hi + 8 lo + 64 r, stored at k + (k >> 3) = hi + 9 lo + 72 r: the
            s_fft[hi + 9 * lo + 72 * r] = v[r];   // plain index is a 4-way bank conflict (lo strides 16 words), the padded one 1-2 way
        }
        wave_sync();

        // real-FFT split: X[k] = E[k] + W_1024^k O[k], X[512-k] = conj(E[k] - W_1024^k O[k])
        float pk[4], pm[4], p256 = 0.f, energy = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = lane + 64 * i;
            const int km = (512 - k) & 511;
            const float2 zk = s_fft[k + (k >> 3)], zm = s_fft[km + (km >> 3)];
            const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            const float2 O = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
            const float2 T = cmul(c.tws[k], O);
            const float2 xp = cadd(E, T), xm = csub(E, T);
            pk[i] = (xp.x * xp.x + xp.y * xp.y) * c.inv_nfft;   // bark_feature.py:88-89
            pm[i] = (xm.x * xm.x + xm.y * xm.y) * c.inv_nfft;
            energy += pk[i] + pm[i];
        }
        if (lane == 0) {  // bin 256 is its own partner
            const float2 z = s_fft[256 + 32];
            p256 = (z.x * z.x + z.y * z.y) * c.inv_nfft;
            energy += p256;
        }
        wave_sync();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = lane + 64 * i;
            s_pw[k] = pk[i];
            s_pw[512 - k] = pm[i];
        }
        if (lane == 0) s_pw[256] = p256;
        energy = wave_sum_dpp(energy);      // VALU-only reduction (6 ds_bpermute round trips otherwise)
        wave_sync();

        // sparse band gather: lane = one chunk (<= chp bins) of one band's non-zero span.  Fixed trip count over
        // zero-padded weights so the LDS loads of a group issue back to back.
        float part = 0.f;
        {
            const float *pp = s_pw + (chunk_pack & 0xFFFF);
            const float *wp = s_w + lane * c.chp;
            for (int t = 0; t < c.chp; t += 4) {
                const float4 wv = *reinterpret_cast<const float4 *>(wp + t);
                const float p0 = pp[t], p1 = pp[t + 1], p2 = pp[t + 2], p3 = pp[t + 3];
                part = fmaf(p0, wv.x, part);
                part = fmaf(p1, wv.y, part);
                part = fmaf(p2, wv.z, part);
                part = fmaf(p3, wv.w, part);
            }
        }
        s_part[qi * 64 + (chunk_pack >> 16)] = part;
        if (lane == 0) s_en[qi] = energy;
        ++qi;
        if (qi < tb && f + 1 < f_end) continue;

        // ---- tail of the qi frames f-qi+1 .. f: band sums -> log -> DCT, all frames of the batch at once ----
        // lane roles are recomputed per batch (twice per wave) rather than held in registers across the FFTs;
        // (lane + 0.5) / n is at least 0.5/64 away from an integer, so the reciprocal multiply floors exactly
        const int f0 = f + 1 - qi;
        int tl = lane;                     // opaque copy: keeps the role arithmetic below inside the tail (it is loop-invariant,
        asm volatile("" : "+v"(tl));     // so the compiler would otherwise hoist it out of the frame loop and spill it)
        wave_sync();
        {
            const int bq = (int)(((float)tl + 0.5f) * r_filt), bm = tl - bq * c.n_filt;       // lane = (frame in batch, band)
            if (bq < qi) {
                const int q0 = s_bcs[bm], cnt = s_bcs[bm + 1] - q0;
                const float *pq = s_part + bq * 64 + q0;
                float sum = 0.f;
                for (int g = 0; g < cnt; g += 8) {                       // reads past cnt stay inside s_part / s_mel and are masked
                    float pv[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) pv[i] = pq[g + i];
#pragma unroll
                    for (int i = 0; i < 8; ++i) sum += (g + i < cnt) ? pv[i] : 0.f;
                }
                s_mel[bq * c.n_filt_pad + bm] = logf(fmaxf(sum, kEps));   // safe_log, bark_feature.py:75-77
            }
        }
        wave_sync();
        {
            const int dq = (int)(((float)tl + 0.5f) * r_out), dn = tl - dq * c.n_out;         // lane = (frame in batch, coefficient)
            if (dq < qi) {
                const float *mq = s_mel + dq * c.n_filt_pad;
                float sum = 0.f;
                for (int n = 0; n < c.n_filt_pad; n += 4) {
                    const float4 mv = *reinterpret_cast<const float4 *>(mq + n);
                    const float d0 = s_dct[n * c.n_out + dn], d1 = s_dct[(n + 1) * c.n_out + dn];
                    const float d2 = s_dct[(n + 2) * c.n_out + dn], d3 = s_dct[(n + 3) * c.n_out + dn];
                    sum = fmaf(mv.x, d0, sum);
                    sum = fmaf(mv.y, d1, sum);
                    sum = fmaf(mv.z, d2, sum);
                    sum = fmaf(mv.w, d3, sum);
                }
                if (dn == 0) sum = logf(fmaxf(s_en[dq], kEps));           // c0 <- log energy, bark_feature.py:173
                if (c.use_delta) s_feat[f0 * c.n_out + tl] = sum;         // lane = dq * n_out + dn
                else dst[f0 * c.n_out + tl] = sum;                        // feature_size == n_out: rows f0.. are contiguous
            }
        }
        qi = 0;
        wave_sync();
    }
    if (!c.use_delta) return;
    __syncthreads();
    dst = feat + (int64_t)blockIdx.x * c.n_frames * c.feature_size;        // with deltas the block is one clip

    // add_deltas (data_utils.py:50-58): the clip's (n_features x 2 n_out) block from the staged coefficients
    const int total = c.n_frames * c.feature_size;
    for (int i = tid; i < total; i += kThreads) {
        const int fr = i / c.feature_size, col = i - fr * c.feature_size;
        float val;
        if (col < c.n_out) val = s_feat[fr * c.n_out + col];
        else val = fr == 0 ? 0.f : s_feat[fr * c.n_out + col - c.n_out] - s_feat[(fr - 1) * c.n_out + col - c.n_out];
        dst[i] = val;
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Generic fallback for n_fft != 1024 (any power of two 64..4096): same block = clip / wave = frames mapping, but a plain
// in-LDS radix-2 FFT of the zero-padded real frame and per-band loops.  Correct for every params.json the reference
// accepts; the tuned kernel above is the one the default geometry (and the benchmark) uses.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kGenWaves = 4;

template <typename WavT>
__global__ __launch_bounds__(kGenWaves * 64) void featurize_generic_kernel(const WavT *__restrict__ wav, int64_t stride,
                                                                           const int32_t *__restrict__ valid_len, int B, FeatDev c,
                                                                           float *__restrict__ feat)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    if (b >= B) return;
    const int N = c.n_fft, nb = N / 2 + 1;
    float2 *z = reinterpret_cast<float2 *>(smem) + (size_t)wave * N;                       // [N] complex per wave
    float *s_mel = reinterpret_cast<float *>(smem + (size_t)kGenWaves * N * 8) + wave * 64;
    float *s_feat = reinterpret_cast<float *>(smem + (size_t)kGenWaves * N * 8 + kGenWaves * 256);

    const int row = c.index ? c.index[b] : b;
    int len = valid_len ? valid_len[row] : (stride > c.max_samples ? c.max_samples : (int)stride);
    len = len < 0 ? 0 : len;
    if ((int64_t)len > stride) len = (int)stride;
    if (len > c.max_samples) len = c.max_samples;
    const int pad = c.max_samples - len;
    const WavT *src = wav + (int64_t)row * stride;

    for (int f = wave; f < c.n_frames; f += kGenWaves) {
        const int base = f * c.hop;
        for (int i = lane; i < N; i += 64) {                       // bit-reversed load of the (cropped / zero-padded) frame
            const int p = base + i;
            const float v = (i < c.window_eff && p >= pad) ? to_f32(src[p - pad]) : 0.f;
            z[__brev((unsigned)i) >> (32 - c.log2n)] = make_float2(v, 0.f);
        }
        wave_sync();
        for (int st = 1; st <= c.log2n; ++st) {                    // radix-2 decimation in time
            const int half = 1 << (st - 1), tstep = N >> st;
            for (int i = lane; i < N / 2; i += 64) {
                const int k = i & (half - 1), j = ((i >> (st - 1)) << st) + k;
                const float2 w = c.twg[k * tstep], u = z[j], t = cmul(w, z[j + half]);
                z[j] = cadd(u, t);
                z[j + half] = csub(u, t);
            }
            wave_sync();
        }
        float e = 0.f;
        float *pw = reinterpret_cast<float *>(z);                  // power spectrum overwrites the low half in place
        for (int k0 = 0; k0 < nb; k0 += 64) {
            const int k = k0 + lane;
            float pk = 0.f;
            if (k < nb) { const float2 x = z[k]; pk = (x.x * x.x + x.y * x.y) * c.inv_nfft; }
            wave_sync();                                           // every lane has read its z[k] of this group
            if (k < nb) pw[k] = pk;
            e += pk;
        }
        e = wave_sum(e);
        wave_sync();
        float melv = 0.f;
        if (lane < c.n_filt) {
            const float *w = c.bw + (size_t)lane * nb + c.bfirst[lane];
            const float *pp = pw + c.bfirst[lane];
            float sacc = 0.f;
            for (int t = 0; t < c.bwidth[lane]; ++t) sacc = fmaf(pp[t], w[t], sacc);
            melv = logf(fmaxf(sacc, kEps));
        }
        s_mel[lane] = melv;
        wave_sync();
        if (lane < c.n_out) {
            float sacc = 0.f;
            for (int n = 0; n < c.n_filt; ++n) sacc = fmaf(s_mel[n], c.dct[n * c.n_out + lane], sacc);
            if (lane == 0) sacc = logf(fmaxf(e, kEps));
            s_feat[f * c.n_out + lane] = sacc;
        }
        wave_sync();
    }
    __syncthreads();
    float *dst = feat + (int64_t)b * c.n_frames * c.feature_size;
    const int total = c.n_frames * c.feature_size;
    for (int i = tid; i < total; i += kGenWaves * 64) {
        const int fr = i / c.feature_size, col = i - fr * c.feature_size;
        float val;
        if (col < c.n_out) val = s_feat[fr * c.n_out + col];
        else val = fr == 0 ? 0.f : s_feat[fr * c.n_out + col - c.n_out] - s_feat[(fr - 1) * c.n_out + col - c.n_out];
        dst[i] = val;
    }
}

}  // namespace kws
#include "kws_featurize_v3.h"
namespace kws {

// ---------------------------------------------------------------------------------------------
// host side: job shapes, LDS sizes and launches (the tables themselves: kws_featurize_tables.h)
// ---------------------------------------------------------------------------------------------
constexpr size_t kMaxLdsBytes = 160 * 1024;      // LDS per workgroup on gfx950

// wave jobs of the n_fft = 1024 kernel: fpw consecutive frames of one clip.  Long clips: an equal share per wave of a block;
// short ones (a streaming step has 2 frames per stream): a whole tail batch per job so that one wave serves a stream
static void feat_job_shape(FeatDev &d)
{
    d.fpw = (d.n_frames + kWaves - 1) / kWaves;
    if (!d.use_delta) d.fpw = std::max(d.fpw, std::min(d.n_frames, d.tail_batch));
    d.fpw = std::max(1, d.fpw);
    d.jpc = std::max(1, (d.n_frames + d.fpw - 1) / d.fpw);
}

static size_t generic_smem_bytes(const FeatDev &d)
{
    return (size_t)kGenWaves * d.n_fft * 8 + kGenWaves * 256 + 4 * (size_t)round4(d.n_frames * d.n_out);
}

static size_t feat_smem_bytes(const FeatDev &d)
{
    return (size_t)kWaves * (kFftTile * 8 + 4 * (d.tail_batch * 64 + 64 + 4)) +
           4 * (size_t)(round4(d.n_filt_pad * d.n_out) + round4(d.nnz)) + 8 * (7 * 64 + 7 * 8) + 272 +
           (d.use_delta ? 4 * (size_t)round4(d.n_frames * d.n_out) : 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// kws_featurize_long for the geometries the tuned kernel does not cover: the recordings are cut into segments of `tile` frames
// ((tile - 1) hop + window samples, consecutive segments overlapping by window - hop), the segments go through the clip kernels
// above as a batch of clips of exactly that length (vectorize_raw of each), and their rows are put in place.
// ---------------------------------------------------------------------------------------------------------------------
template <typename WavT>
__global__ __launch_bounds__(256) void long_segments_kernel(const WavT *__restrict__ wav, int64_t stride, const int32_t *__restrict__ lengths,
                                                            int jpc, int64_t seg_step, int seg_len, int64_t total, WavT *__restrict__ seg)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t sg = i / seg_len;
        const int o = (int)(i - sg * seg_len);
        const int r = (int)(sg / jpc);
        const int64_t p = (sg - (int64_t)r * jpc) * seg_step + o;              // sample of recording r; zeros past its end
        int64_t len = lengths[r];
        len = len > stride ? stride : len;
        seg[i] = p < len ? wav[(int64_t)r * stride + p] : (WavT)0;
    }
}

// rows (R, max_frames, D) from the segments' rows (R, jpc * tile, D); zeros past each recording's own frame count
__global__ __launch_bounds__(256) void long_rows_kernel(const float *__restrict__ seg_rows, const int32_t *__restrict__ lengths, int64_t stride,
                                                        int window, int hop, int max_frames, int64_t seg_frames, int D, int64_t total,
                                                        float *__restrict__ rows)
{
    const int64_t per = (int64_t)max_frames * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / per);
        const int64_t o = i - (int64_t)r * per;
        int64_t len = lengths[r];
        len = len > stride ? stride : len;
        const int64_t nf = len < window ? 0 : (len - window) / hop + 1;
        rows[i] = o < nf * D ? seg_rows[(int64_t)r * seg_frames * D + o] : 0.f;
    }
}

}  // namespace kws

using namespace kws;

// tuned kernel (kws_featurize_v3.h): default frame geometry, 20 bands, 20 coefficients, no deltas
constexpr int kTunedBands = 20, kTunedCoefs = 20;
static bool v3_applies(const FeatDev &d)
{
    return d.n_fft == 1024 && d.hop == 512 && d.window_eff == 1024 && !d.use_delta && d.n_filt == kTunedBands && d.n_out == kTunedCoefs &&
           (d.chp3 == 12 || d.chp3 == 16 || d.chp3 == 20);
}
static size_t v3_smem_bytes(int chp, int waves)
{
    constexpr int TB = 64 / kTunedBands;
    return (size_t)waves * 4 * (kV3Tile + TB * 64 + 64 + 4) + 4 * (size_t)(kTunedBands * kTunedCoefs + 64 * chp) + 8 * (size_t)(7 * 64 + 7 * 8 + 4 * 64) +
           4 * (size_t)round4(kTunedBands + 1);
}
// LONG (kws_featurize_long): B recordings of d.n_frames output rows each, valid_len = their sample counts (kws_featurize_v3.h)
template <typename WavT, int CHP, int WAVES, bool AUG = false, bool LONG = false>
static int launch_v3(const FeatDev &d, const WavT *wav, int B, int64_t stride, const int32_t *valid_len, float *feat, hipStream_t s, const char *name, int bpc,
                     const AugDev &aug = {})
{
    const int cus = device_cus();
    const size_t smem = v3_smem_bytes(CHP, WAVES);
    if ((size_t)WAVES * 4 * kV3Tile > 65536) return fail(KWS_ERR_UNSUPPORTED, "wave tiles must sit in the first 64 KiB of LDS (M0 holds 16 address bits)");
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&featurize_fft1024_v3_kernel<WavT, CHP, kTunedBands, kTunedCoefs, WAVES, AUG, LONG>), (int)smem)) return rc;
    FeatDev dd = d;
    const long waves = (long)bpc * cus * WAVES;
    if constexpr (LONG) {
        // a job is a tile of fpw rows of one recording: one round of jobs over the grid's waves when the audio allows it (a one-hour
        // recording is 112 499 frames = 28 per wave of 256 CUs x 16 waves), whole tail batches, at least 4 of them so that a job's fixed
        // part (half a frame of loads, the table reads) stays under a tenth of it, at most 32 so that ragged batches still balance
        const int tb = std::max(1, dd.tail_batch);
        const long total = (long)B * dd.n_frames;
        long fpw = (total + waves - 1) / waves;
        fpw = (fpw + tb - 1) / tb * tb;
        fpw = std::min<long>(std::max<long>(fpw, 4 * tb), 32 * tb);
        dd.fpw = (int)fpw;
        dd.jpc = (dd.n_frames + dd.fpw - 1) / dd.fpw;
    } else {
        // cost of a candidate = rounds of jobs per wave x (frames per job + the job's fixed part: one extra half frame of loads
        // and a partly filled tail batch); candidates: the tail batch size and up, preferring divisors of the frame count
        double best = -1.0;
        for (int fpw = std::min(dd.n_frames, std::max(1, dd.tail_batch)); fpw <= dd.n_frames; ++fpw) {
            const int jpc = (dd.n_frames + fpw - 1) / fpw;
            const long jobs = (long)B * jpc, rounds = (jobs + waves - 1) / waves;
            const double cost = (double)rounds * ((double)fpw + 1.25) + ((dd.n_frames % fpw) ? 0.5 : 0.0);
            if (best < 0 || cost < best - 1e-9) { best = cost; dd.fpw = fpw; dd.jpc = jpc; }
        }
    }
    const long jobs = (long)B * dd.jpc;
    if (jobs > 0x7fffffffL) return fail(KWS_ERR_UNSUPPORTED, "%ld featurizer jobs exceed the kernel's 32-bit job index", jobs);
    const unsigned grid = (unsigned)std::min<long>((long)bpc * cus, (jobs + WAVES - 1) / WAVES);
    KWS_LAUNCH(name, (featurize_fft1024_v3_kernel<WavT, CHP, kTunedBands, kTunedCoefs, WAVES, AUG, LONG>), dim3(grid), dim3(WAVES * 64), smem, s, wav, stride,
               valid_len, B, dd, feat, aug);      // aug is {} (the kernel's default) unless AUG
    KWS_LAUNCH_CHECK("featurize_fft1024_v3_kernel");
    return KWS_OK;
}
constexpr int kV3AloneWaves = 8, kV3AloneBlocks = 2;
template <typename WavT, int WAVES, bool AUG = false, bool LONG = false>
static int launch_v3_chp(const FeatDev &d, const WavT *wav, int B, int64_t stride, const int32_t *valid_len, float *feat, hipStream_t s, const char *name, int bpc,
                         const AugDev &aug = {})
{
    switch (d.chp3) {
    case 12: return launch_v3<WavT, 12, WAVES, AUG, LONG>(d, wav, B, stride, valid_len, feat, s, name, bpc, aug);
    case 16: return launch_v3<WavT, 16, WAVES, AUG, LONG>(d, wav, B, stride, valid_len, feat, s, name, bpc, aug);
    default: return launch_v3<WavT, 20, WAVES, AUG, LONG>(d, wav, B, stride, valid_len, feat, s, name, bpc, aug);
    }
}
// The kernel holds its per-lane twiddles in registers (110 registers: 4 waves per SIMD = 16 per CU).  With the chip to itself: two blocks of 8
// waves per CU; beside a train step (kws_featurizer_set_cu_share(f, 1)): ONE block of 12 waves per CU, which leaves a quarter of the wave
// slots and half of the LDS to the step's kernels.
template <typename WavT, bool AUG = false, bool LONG = false>
static int launch_v3_any(const FeatDev &d, const WavT *wav, int B, int64_t stride, const int32_t *valid_len, float *feat, hipStream_t s, const char *name,
                         const AugDev &aug = {})
{
    if (d.blocks_per_cu == 1) return launch_v3_chp<WavT, kV3Waves, AUG, LONG>(d, wav, B, stride, valid_len, feat, s, name, 1, aug);
    return launch_v3_chp<WavT, kV3AloneWaves, AUG, LONG>(d, wav, B, stride, valid_len, feat, s, name, kV3AloneBlocks, aug);
}

// f(const float *) or f(const short *) for the samples at wav: the one place that reads wav_dtype.  Its return type and the lambdas'
// are deduced, so they are instantiated where they are written and the kernels stay in the code object in source order.
template <typename F> static auto with_wav(int wav_dtype, const void *wav, F &&f)
{
    if (wav_dtype == KWS_WAV_F32) return f(static_cast<const float *>(wav));
    if (wav_dtype == KWS_WAV_I16) return f(static_cast<const short *>(wav));
    return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
}
template <typename P> using wav_type = std::remove_cv_t<std::remove_pointer_t<P>>;
// the launch's name in profiles: one per sample type
template <typename WavT> static const char *wav_name(const char *name_f32, const char *name_i16) { return std::is_same<WavT, float>::value ? name_f32 : name_i16; }

// the tables seen as "rows of n_frames frames from max_samples samples, no deltas": raw audio, long recordings and their segments
static FeatDev rows_view(const kws_featurizer *f, int n_frames, int max_samples)
{
    FeatDev d = f->dev;
    d.n_frames = n_frames; d.max_samples = max_samples; d.use_delta = 0; d.feature_size = d.n_out;
    d.blocks_per_cu = f->blocks_per_cu; d.index = nullptr;
    return d;
}

// the first-generation or the generic kernel on B clips: its dynamic LDS, the launch, its status
template <typename WavT>
static int launch_clips(const char *name, const char *what, void (*kernel)(const WavT *, int64_t, const int32_t *, int, FeatDev, float *), dim3 grid, dim3 block,
                        size_t smem, hipStream_t s, const WavT *wav, int64_t stride, const int32_t *valid_len, int B, const FeatDev &d, float *feat)
{
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (int)smem)) return rc;
    KWS_LAUNCH(name, kernel, grid, block, smem, s, wav, stride, valid_len, B, d, feat);
    KWS_LAUNCH_CHECK(what);
    return KWS_OK;
}

static int launch_generic(const FeatDev &d, const void *wav, int wav_dtype, int B, int64_t stride, const int32_t *valid_len, float *feat, void *stream)
{
    const size_t smem = generic_smem_bytes(d);
    if (smem > kMaxLdsBytes) return fail(KWS_ERR_UNSUPPORTED, "n_fft=%d with %d frames needs %zu B of LDS (> 160 KiB)", d.n_fft, d.n_frames, smem);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_wav(wav_dtype, wav, [&](auto *w) {
        using WavT = wav_type<decltype(w)>;
        return launch_clips(wav_name<WavT>("featurize_generic_f32", "featurize_generic_i16"), "featurize_generic_kernel", featurize_generic_kernel<WavT>,
                            dim3((unsigned)B), dim3(kGenWaves * 64), smem, s, w, stride, valid_len, B, d, feat);
    });
}

static int launch_featurize(const FeatDev &d0, const void *wav, int wav_dtype, int B, int64_t stride, const int32_t *valid_len, float *feat, void *stream)
{
    if (d0.n_fft != 1024) return launch_generic(d0, wav, wav_dtype, B, stride, valid_len, feat, stream);
    FeatDev d = d0;
    feat_job_shape(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (v3_applies(d))
        return with_wav(wav_dtype, wav, [&](auto *w) {
            return launch_v3_any(d, w, B, stride, valid_len, feat, s, wav_name<wav_type<decltype(w)>>("featurize_fft1024_f32", "featurize_fft1024_i16"));
        });
    const size_t smem = feat_smem_bytes(d);
    if (smem > kMaxLdsBytes) return fail(KWS_ERR_UNSUPPORTED, "%d frames need %zu B of LDS (> 160 KiB)", d.n_frames, smem);
    const long jobs = (long)B * d.jpc;
    const dim3 grid((unsigned)(d.use_delta ? B : (jobs + kWaves - 1) / kWaves));
    return with_wav(wav_dtype, wav, [&](auto *w) {
        using WavT = wav_type<decltype(w)>;
        return launch_clips(wav_name<WavT>("featurize_fft1024_f32", "featurize_fft1024_i16"), "featurize_fft1024_kernel", featurize_fft1024_kernel<WavT>, grid,
                            dim3(kThreads), smem, s, w, stride, valid_len, B, d, feat);
    });
}

// kws_featurize_long off the tuned kernel's geometry (long_segments_kernel / long_rows_kernel above)
template <typename WavT>
static int featurize_long_segments(const kws_featurizer *f, const WavT *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths,
                                   int max_frames, float *rows, hipStream_t s)
{
    const int window = f->geom.window_samples, hop = f->geom.hop_samples, D = f->dev.n_out;
    // frames per segment: what the generic kernel can stage in LDS beside its FFT tiles, 256 at the most
    int tile = 256;
    if (f->dev.n_fft != 1024) {
        const size_t fixed = (size_t)kGenWaves * f->dev.n_fft * 8 + kGenWaves * 256;
        tile = (int)std::min<size_t>(256, (kMaxLdsBytes - fixed) / (4 * (size_t)D) - 4);
    }
    tile = std::max(1, std::min(tile, max_frames));
    const int jpc = (max_frames + tile - 1) / tile;
    const int64_t seg_len = (int64_t)(tile - 1) * hop + window, n_seg = (int64_t)R * jpc;
    if (n_seg > 0x7fffffffL || seg_len > 0x7fffffffL) return fail(KWS_ERR_UNSUPPORTED, "%lld segments of %lld samples", (long long)n_seg, (long long)seg_len);
    const size_t seg_bytes = (sizeof(WavT) * (size_t)n_seg * seg_len + 255) & ~(size_t)255;
    unsigned char *tmp = nullptr;
    KWS_HIP_CHECK(hipMallocAsync(reinterpret_cast<void **>(&tmp), seg_bytes + sizeof(float) * (size_t)n_seg * tile * D, s));
    WavT *seg = reinterpret_cast<WavT *>(tmp);
    float *seg_rows = reinterpret_cast<float *>(tmp + seg_bytes);
    const int64_t n_in = n_seg * seg_len, n_out = (int64_t)R * max_frames * D;
    const int cap = 64 * device_cus();
    KWS_LAUNCH("long_segments_kernel", long_segments_kernel<WavT>, dim3((unsigned)std::min<int64_t>(cap, (n_in + 255) / 256)), dim3(256), 0, s, wav, stride,
               lengths, jpc, (int64_t)tile * hop, (int)seg_len, n_in, seg);
    KWS_LAUNCH_CHECK("long_segments_kernel");
    int rc = launch_featurize(rows_view(f, tile, (int)seg_len), seg, wav_dtype, (int)n_seg, seg_len, nullptr, seg_rows, s);
    if (rc == KWS_OK) {
        KWS_LAUNCH("long_rows_kernel", long_rows_kernel, dim3((unsigned)std::min<int64_t>(cap, (n_out + 255) / 256)), dim3(256), 0, s, seg_rows, lengths,
                   stride, window, hop, max_frames, (int64_t)jpc * tile, D, n_out, rows);
        KWS_LAUNCH_CHECK("long_rows_kernel");
    }
    KWS_HIP_CHECK(hipFreeAsync(tmp, s));
    return rc;
}

// a builder's status with its message (kws_featurize_tables.h) as this library reports errors
static int table_status(int rc, const std::string &err) { return rc ? fail(rc, "%s", err.c_str()) : KWS_OK; }

extern "C" {

void kws_params_default(kws_params *p)
{
    if (!p) return;
    // classifier/params.py:99-103
    p->buffer_t = 1.0; p->window_t = 0.064; p->hop_t = 0.032;
    p->sample_rate = 16000; p->sample_depth = 2; p->n_fft = 1024; p->n_filt = 20; p->n_mfcc = 20; p->use_delta = 0;
}

int kws_params_derive(const kws_params *p, kws_geometry *g) { std::string err; return table_status(derive(p, g, err), err); }

int kws_featurizer_create(const kws_params *p, int bank_kind, kws_featurizer **out)
{
    if (!p || !out) return fail(KWS_ERR_INVALID, "null argument");
    *out = nullptr;
    kws_geometry g;
    if (int rc = kws_params_derive(p, &g)) return rc;
    if (bank_kind != KWS_BANK_MEL && bank_kind != KWS_BANK_BARK) return fail(KWS_ERR_INVALID, "unknown bank kind %d", bank_kind);
    if (p->n_filt < 1 || p->n_filt > 64) return fail(KWS_ERR_UNSUPPORTED, "n_filt must be in 1..64, got %d", p->n_filt);
    if (p->n_mfcc < 1 || p->n_mfcc > p->n_filt)
        return fail(KWS_ERR_INVALID, "n_mfcc=%d must be in 1..n_filt=%d (the reference's feature_size would not match)", p->n_mfcc, p->n_filt);
    if (p->n_fft < 64 || p->n_fft > 4096 || (p->n_fft & (p->n_fft - 1)))
        return fail(KWS_ERR_UNSUPPORTED, "n_fft must be a power of two in 64..4096 (got %d)", p->n_fft);
    if (g.max_samples < g.window_samples) return fail(KWS_ERR_INVALID, "buffer shorter than one window");
    if (clip_frames(g) != g.n_features)
        return fail(KWS_ERR_INVALID, "params give %d frames but n_features=%d; the reference's model input would not match", clip_frames(g), g.n_features);

    FeatTables t;
    std::string err;
    if (int rc = build_feat_tables(*p, g, bank_kind, t, err)) return table_status(rc, err);
    std::unique_ptr<kws_featurizer, decltype(&kws_featurizer_destroy)> f(new kws_featurizer(), kws_featurizer_destroy);
    f->params = *p; f->geom = g; f->bank_kind = bank_kind; f->bank = t.bw;
    FeatDev &d = f->dev;
    // the device image: every table once, in the order the kernels have always found them
    TableArena arena;
    arena.add(t.tw1, &d.tw1);
    arena.add(t.tw2, &d.tw2);
    arena.add(t.tws, &d.tws);
    arena.add(t.T1.chunks, &d.chunks, 1);
    arena.add(t.T1.bcs, &d.bcs);
    arena.add(t.T1.w, &d.w, 1);
    arena.add(t.dct, &d.dct);
    arena.add(t.twg, &d.twg);
    arena.add(t.first, &d.bfirst);
    arena.add(t.width, &d.bwidth);
    arena.add(t.bw, &d.bw);
    arena.add(t.T3.chunks, &d.chunks3);
    arena.add(t.T3.bcs, &d.bcs3);
    arena.add(t.T3.w, &d.w3);
    arena.add(t.tw1s, &d.tw1s);
    arena.add(t.tws3, &d.tws3);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(KWS_ERR_HIP, "no HIP device: the featurizer has no CPU fallback");
    }
    hipError_t e = hipMalloc(&f->dmem, arena.image.size());
    if (e == hipSuccess) e = hipMemcpy(f->dmem, arena.image.data(), arena.image.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(KWS_ERR_HIP, "featurizer table upload failed: %s", hipGetErrorString(e));
    arena.bind(f->dmem);

    d.window_eff = t.window_eff; d.hop = g.hop_samples; d.max_samples = g.max_samples; d.n_frames = t.n_frames;
    d.n_filt = p->n_filt; d.n_out = p->n_mfcc; d.feature_size = g.feature_size; d.use_delta = p->use_delta ? 1 : 0;
    d.nchunks = t.T1.nlog; d.nnz = (int)t.T1.w.size(); d.inv_nfft = 1.0f / (float)p->n_fft;
    d.chp = t.T1.chp; d.n_filt_pad = t.n_filt_pad; d.tail_batch = t.tail_batch;
    d.n_fft = p->n_fft; d.log2n = t.log2n;
    d.chp3 = (p->n_fft == 1024 && t.T3.nlog <= 64) ? t.T3.chp : 0;
    // the LDS the launch will ask for (same job shape as launch_featurize / launch_generic, same 160 KiB limit)
    if (d.n_fft == 1024) feat_job_shape(d);
    f->smem_bytes = d.n_fft == 1024 ? feat_smem_bytes(d) : generic_smem_bytes(d);
    if (f->smem_bytes > kMaxLdsBytes)
        return fail(KWS_ERR_UNSUPPORTED, "featurizer needs %zu B of LDS per block (> %d KiB)", f->smem_bytes, (int)(kMaxLdsBytes / 1024));
    *out = f.release();
    return KWS_OK;
}

void kws_featurizer_destroy(kws_featurizer *f)
{
    if (!f) return;
    if (f->dmem) (void)hipFree(f->dmem);
    delete f;
}

int kws_featurizer_geometry(const kws_featurizer *f, kws_geometry *g)
{
    if (!f || !g) return fail(KWS_ERR_INVALID, "null argument");
    *g = f->geom;
    return KWS_OK;
}

int kws_featurizer_bank(const kws_featurizer *f, float *host_bank, size_t count)
{
    if (!f || !host_bank) return fail(KWS_ERR_INVALID, "null argument");
    if (count != f->bank.size()) return fail(KWS_ERR_INVALID, "bank has %zu floats, caller asked for %zu", f->bank.size(), count);
    std::memcpy(host_bank, f->bank.data(), count * sizeof(float));
    return KWS_OK;
}

int kws_featurize_gather(kws_featurizer *f, const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride,
                         const int32_t *valid_len, float *feat, void *stream)
{
    if (!f || !feat || (!wav && B > 0)) return fail(KWS_ERR_INVALID, "null argument");
    if (B < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative batch or stride");
    if (B == 0) return KWS_OK;
    if (!valid_len && stride < 1) return fail(KWS_ERR_INVALID, "stride must be >= 1 when valid_len is NULL");
    FeatDev d = f->dev;
    d.blocks_per_cu = f->blocks_per_cu;
    d.index = index;
    return launch_featurize(d, wav, wav_dtype, B, stride, valid_len, feat, stream);
}

int kws_featurize_gather_augmented(kws_featurizer *f, const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride,
                                   const kws_noise_bank *bank, const kws_aug_clip *plan, float *feat, void *stream)
{
    if (!f || !feat || !bank || (B > 0 && (!wav || !plan))) return fail(KWS_ERR_INVALID, "null argument");
    if (B < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative batch or stride");
    if (bank->K < 1) return fail(KWS_ERR_INVALID, "empty noise bank");
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    if (B == 0) return KWS_OK;
    FeatDev d = f->dev;
    d.blocks_per_cu = f->blocks_per_cu;
    d.index = index;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d.n_fft == 1024) {
        feat_job_shape(d);
        if (v3_applies(d)) {       // the default geometry: the mix happens in the tuned kernel's sample loads
            const AugDev aug{plan, bank->samples, bank->d_start};
            return with_wav(wav_dtype, wav, [&](auto *w) {
                using WavT = wav_type<decltype(w)>;
                return launch_v3_any<WavT, true>(d, w, B, stride, nullptr, feat, s, wav_name<WavT>("featurize_fft1024_aug_f32", "featurize_fft1024_aug_i16"), aug);
            });
        }
    }
    // other geometries: materialise the clips (stream-ordered scratch), then the plain featurizer on them with valid_len = L
    const int ms = f->dev.max_samples;
    float *tmp = nullptr;
    KWS_HIP_CHECK(hipMallocAsync(reinterpret_cast<void **>(&tmp), sizeof(float) * (size_t)B * ms + sizeof(int32_t) * (size_t)B, s));
    int32_t *lens = reinterpret_cast<int32_t *>(tmp + (size_t)B * ms);
    int rc = augment_apply_launch(bank, plan, wav, wav_dtype, index, B, stride, ms, tmp, ms, lens, s);
    if (rc == KWS_OK) {
        d = f->dev;
        d.blocks_per_cu = f->blocks_per_cu;
        rc = launch_featurize(d, tmp, KWS_WAV_F32, B, ms, lens, feat, stream);
    }
    KWS_HIP_CHECK(hipFreeAsync(tmp, s));
    return rc;
}

int kws_featurize(kws_featurizer *f, const void *wav, int wav_dtype, int B, int64_t stride, const int32_t *valid_len,
                  float *feat, void *stream)
{
    return kws_featurize_gather(f, wav, wav_dtype, nullptr, B, stride, valid_len, feat, stream);
}

int kws_featurizer_set_cu_share(kws_featurizer *f, int blocks_per_cu)
{
    if (!f) return fail(KWS_ERR_INVALID, "null argument");
    if (blocks_per_cu != 1 && blocks_per_cu != 2) return fail(KWS_ERR_INVALID, "blocks_per_cu must be 1 or 2");
    f->blocks_per_cu = blocks_per_cu;
    return KWS_OK;
}

int kws_featurizer_occupancy(const kws_featurizer *f, int *blocks_per_cu, size_t *lds_bytes)
{
    if (!f || !blocks_per_cu) return fail(KWS_ERR_INVALID, "null argument");
    const bool tuned = f->dev.n_fft == 1024;
    const size_t smem = f->smem_bytes;
    if (lds_bytes) *lds_bytes = smem;
    int nb = 0;
    // n_fft = 1024 reports the first-generation kernel even where the tuned one (launch_v3) runs: odd, but callers have always seen it
    if (tuned)
        KWS_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, featurize_fft1024_kernel<float>, kThreads, smem));
    else
        KWS_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, featurize_generic_kernel<float>, kGenWaves * 64, smem));
    *blocks_per_cu = nb;
    return KWS_OK;
}

int kws_featurize_raw_frames(const kws_featurizer *f, int32_t n_samples)
{
    if (!f || n_samples < f->geom.window_samples) return 0;  // chop_array, bark_feature.py:80-82
    return (n_samples - f->geom.window_samples) / f->geom.hop_samples + 1;
}

int kws_featurize_raw(kws_featurizer *f, const void *wav, int wav_dtype, int B, int64_t stride, int32_t n_samples,
                      float *feat, void *stream)
{
    if (!f || !feat || (!wav && B > 0)) return fail(KWS_ERR_INVALID, "null argument");
    if (B < 0 || n_samples < 0 || stride < n_samples) return fail(KWS_ERR_INVALID, "bad batch / n_samples / stride");
    const int n_frames = kws_featurize_raw_frames(f, n_samples);
    if (B == 0 || n_frames == 0) return KWS_OK;  // sonopy returns an empty matrix
    return launch_featurize(rows_view(f, n_frames, n_samples), wav, wav_dtype, B, stride, nullptr, feat, stream);
}

int kws_featurize_long(kws_featurizer *f, const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths, int max_frames,
                       float *rows, void *stream)
{
    if (!f) return fail(KWS_ERR_INVALID, "null argument");
    if (R < 0 || max_frames < 0 || stride < 0) return fail(KWS_ERR_INVALID, "negative R / max_frames / stride");
    if (wav_dtype != KWS_WAV_F32 && wav_dtype != KWS_WAV_I16) return fail(KWS_ERR_INVALID, "unknown wav dtype %d", wav_dtype);
    if (R == 0 || max_frames == 0) return KWS_OK;
    if (!wav || !lengths || !rows) return fail(KWS_ERR_INVALID, "null argument");
    // lengths are int32, so a recording has fewer than 2^31 / hop frames; the kernels index samples and row elements with 32 bits
    if ((int64_t)max_frames * std::max(f->geom.hop_samples, f->dev.n_out) > 0x7fffffffL - f->geom.window_samples)
        return fail(KWS_ERR_INVALID, "max_frames=%d is more than an int32 sample count can hold", max_frames);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FeatDev d = rows_view(f, max_frames, f->dev.max_samples);
    feat_job_shape(d);
    if (d.n_fft == 1024 && v3_applies(d))      // the default geometry: tiles of frames are the tuned kernel's own jobs
        return with_wav(wav_dtype, wav, [&](auto *w) {
            using WavT = wav_type<decltype(w)>;
            return launch_v3_any<WavT, false, true>(d, w, R, stride, lengths, rows, s, wav_name<WavT>("featurize_long_f32", "featurize_long_i16"));
        });
    return with_wav(wav_dtype, wav, [&](auto *w) { return featurize_long_segments(f, w, wav_dtype, R, stride, lengths, max_frames, rows, s); });
}

}  // extern "C"
