// csrc/kws_transfer.hip -- kws_head_fit: Dense(E -> C, softmax) heads trained on frozen embeddings, every step of a head inside one
// block of one launch (include/kws.h).
//
// One 256-thread block per job.  The kernel matrix is padded to CP = the next power of two >= C columns and dealt to the threads so that
// each owns its elements for the whole launch: thread t owns column c = t % CP and the rows e = eg + k * ES, eg = t / CP, ES = 256 / CP,
// k < EPT.  The owner keeps the weight, its optimizer slots and its gradient sum in registers -- nothing of a job's state lives in memory
// between its first load and its last store -- and the products of a step are "owner computes":
//   logits   every thread multiplies ITS rows of W into the tile's rows of X, the ES partial sums of an output meet in LDS and are added
//            in the order eg = 0, 1, ..;
//   dW       every thread adds X[r][e] * dlogits[r][c] for ITS (e, c), row after row.
// A step's batch is walked in tiles of 16 rows gathered by `order` into a double-buffered LDS tile: the loads of the next tile (across the
// step boundary too: X does not depend on the weights) are issued before the current tile's math and stored behind it.  Every sum has one
// fixed order, there are no atomics and blocks never talk to each other, so a job's bits do not depend on J, on the other jobs or on the run.
// Multiply-adds are spelled out (fmaf) and contraction is off, so that the instantiations (EPT follows the widest job of a launch)
// compute the same bits.
#include <cmath>

#include "kws_common.h"

namespace kws {

namespace {

constexpr int kHfThreads = 256;
constexpr int kHfRows = 16;              // rows of a tile
constexpr int kHfMaxE = 128;
constexpr int kHfMaxEpt = 32;            // elements of the kernel matrix per thread and register array (w, m, v, dW)
constexpr int kHfMaxCp = 256;            // padded classes: one column per thread at most
constexpr int kLdsPerCu = 160 * 1024;
constexpr float kHfCeEps = 1e-7f;        // keras.backend.epsilon()

inline int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }
// LDS of a block with CP padded classes: two X tiles, the partial sums, the logits tile, the bias, labels and per-row results
inline size_t hf_lds_bytes(int E, int cp) { return sizeof(float) * ((size_t)2 * kHfRows * E + (size_t)kHfRows * kHfThreads + (size_t)kHfRows * cp + cp + 4 * kHfRows); }

struct HfShared {
    float x[2][kHfRows * kHfMaxE];
    float part[kHfRows * kHfThreads];
    float lg[kHfRows * kHfMaxCp];
    float bias[kHfMaxCp];
    int y[2][kHfRows];
    float row_loss[kHfRows], row_hit[kHfRows];
};

// rows [row0, row0 + cnt) of a job's order slice: the next tile to gather
struct HfTile { int row0, cnt; };

template <int EPT>
__global__ __launch_bounds__(kHfThreads) void head_fit_kernel(const float *__restrict__ emb, const int32_t *__restrict__ labels, int E,
                                                               const int32_t *__restrict__ order, const float *__restrict__ class_w,
                                                               const kws_head_job *__restrict__ jobs, float *__restrict__ weights,
                                                               float *__restrict__ slot_m, float *__restrict__ slot_v,
                                                               float *__restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ HfShared sh;
    const kws_head_job job = jobs[blockIdx.x];
    const int n = job.n_order;
    if (n <= 0) return;                                     // the job is left exactly as given
    const int t = threadIdx.x, C = job.num_classes, batch = job.batch;
    int cp = 2;
    while (cp < C) cp <<= 1;
    const int es = kHfThreads / cp, c = t & (cp - 1), eg = t / cp;
    const int nk = (eg < E && c < C) ? (E - eg + es - 1) / es : 0;      // elements this thread owns
    const int egn = es < E ? es : E;                                    // partial sums per output
    const bool own_bias = t < C;                                        // eg == 0, c = t
    const bool adam = job.optimizer == KWS_OPT_ADAM;
    const float *cw = job.class_weight_offset >= 0 ? class_w + job.class_weight_offset : nullptr;
    const int32_t *ord = order + job.order_offset;
    float *wj = weights + job.weight_offset;
    float *mj = slot_m ? slot_m + job.weight_offset : nullptr, *vj = slot_v ? slot_v + job.weight_offset : nullptr;

    // rows of a tile that are in flight together: as many as the registers beside the four EPT-long arrays allow without scratch
    constexpr int RG = EPT <= 4 ? 4 : (EPT <= 16 ? 2 : 1);
    float w[EPT], m[EPT], v[EPT], acc[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = (long)(eg + k * es) * C + c;
        const bool on = k < nk;
        w[k] = on ? wj[i] : 0.f;
        m[k] = on && mj ? mj[i] : 0.f;
        v[k] = on && vj && adam ? vj[i] : 0.f;
    }
    float wb = own_bias ? wj[(long)E * C + t] : 0.f;
    float mb = own_bias && mj ? mj[(long)E * C + t] : 0.f, vb = own_bias && vj && adam ? vj[(long)E * C + t] : 0.f;
    for (int i = t; i < kHfRows * kHfMaxCp; i += kHfThreads) sh.lg[i] = 0.f;       // the padding columns stay zero
    if (t < kHfMaxCp) sh.bias[t] = wb;

    // the gather of one tile: E / 4 float4 per row, at most two per thread, and the row's label
    const int q4 = E / 4, nld = kHfRows * q4;
    float4 px[2];
    int py = 0;
    auto fetch = [&](HfTile tl) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = t + q * kHfThreads, r = i / q4, col = i - r * q4;
            px[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < nld && r < tl.cnt) px[q] = *reinterpret_cast<const float4 *>(emb + (long)ord[tl.row0 + r] * E + 4 * col);
        }
        if (t < kHfRows) py = t < tl.cnt ? labels[ord[tl.row0 + t]] : 0;
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = t + q * kHfThreads;
            if (i < nld) *reinterpret_cast<float4 *>(&sh.x[buf][4 * i]) = px[q];
        }
        if (t < kHfRows) sh.y[buf][t] = py;
    };

    const int steps = (int)(((long)n + batch - 1) / batch);
    fetch(HfTile{0, min(kHfRows, min(batch, n))});
    stash(0);
    __syncthreads();

    double loss_sum = 0.0, hit_sum = 0.0;           // thread 0: row after row, as loss_reduce_kernel sums a step's (in double)
    int buf = 0;
    for (int step = 0; step < steps; ++step) {
        const int base = step * batch, nb = min(batch, n - base), ntile = (nb + kHfRows - 1) / kHfRows;
        const float inv = 1.f / (float)nb;          // d(mean)/d(logits) carries 1 / (rows of THIS step)
#pragma unroll
        for (int k = 0; k < EPT; ++k) acc[k] = 0.f;
        float accb = 0.f;
        for (int ti = 0; ti < ntile; ++ti) {
            const int cnt = min(kHfRows, nb - ti * kHfRows);
            // next tile: of this step, or the first of the next one
            HfTile nx{0, 0};
            if (ti + 1 < ntile) nx = HfTile{base + (ti + 1) * kHfRows, min(kHfRows, nb - (ti + 1) * kHfRows)};
            else if (step + 1 < steps) nx = HfTile{base + batch, min(kHfRows, min(batch, n - base - batch))};
            fetch(nx);
            const float *xs = sh.x[buf];
            // logits, partial over this thread's rows of W
            // (RG rows at a time, their LDS reads issued together: a block has one wave per SIMD and nothing else hides a read's
            // latency; rows past cnt are zeros in the tile.  A k past this thread's elements multiplies a zero weight into a zero)
            const int cnt4 = (cnt + RG - 1) / RG * RG;
            for (int r0 = 0; r0 < cnt4; r0 += RG) {
                float p[RG] = {};
#pragma unroll
                for (int k = 0; k < EPT; ++k) {
                    const int e = eg + k * es;
                    const bool on = e < E;
#pragma unroll
                    for (int j = 0; j < RG; ++j) {
                        const float xv = xs[(r0 + j) * E + (on ? e : 0)];
                        p[j] = fmaf(on ? xv : 0.f, w[k], p[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < RG; ++j) sh.part[(r0 + j) * kHfThreads + t] = p[j];
            }
            __syncthreads();
            // softmax, loss and dlogits: 16 lanes per row, class c2 = lane + 16 i
            {
                const int r = t >> 4, lane = t & 15;
                const bool live = r < cnt;
                float mx = -INFINITY;
                int am = 0x7fffffff;
                if (live)
                    for (int c2 = lane; c2 < C; c2 += 16) {
                        float s = 0.f;
#pragma unroll 4
                        for (int g = 0; g < egn; ++g) s += sh.part[r * kHfThreads + g * cp + c2];
                        s += sh.bias[c2];
                        sh.lg[r * cp + c2] = s;
                        if (s > mx) { mx = s; am = c2; }
                    }
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) {
                    const float omx = __shfl_xor(mx, o, 16);
                    const int oam = __shfl_xor(am, o, 16);
                    if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
                }
                const int y = sh.y[buf][r];
                float sum = 0.f, ey = 0.f;
                if (live)
                    for (int c2 = lane; c2 < C; c2 += 16) {
                        const float e = expf(sh.lg[r * cp + c2] - mx);
                        sh.lg[r * cp + c2] = e;
                        sum += e;
                        if (c2 == y) ey = e;
                    }
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) {
                    sum += __shfl_xor(sum, o, 16);
                    ey += __shfl_xor(ey, o, 16);           // one lane holds e_y, the others zero
                }
                if (live) {
                    const float rs = 1.f / sum, pyv = ey * rs;
                    const bool ignored = job.ignore_index > 0 && y == job.ignore_index;     // its label may lie outside [0, C)
                    float loss, coef;
                    if (ignored) {
                        loss = 0.f;
                        coef = 0.f;
                    } else if (cw) {                         // weighted: -log(p_y) w_y, unclipped
                        loss = -logf(pyv) * cw[y];
                        coef = cw[y];
                    } else {                                 // plain: p_y clipped, the gradient gated by the clip
                        const float lo = kHfCeEps, hi = 1.f - kHfCeEps;
                        loss = -logf(fminf(fmaxf(pyv, lo), hi));
                        coef = (pyv >= lo && pyv <= hi) ? 1.f : 0.f;
                    }
                    for (int c2 = lane; c2 < C; c2 += 16)
                        sh.lg[r * cp + c2] = (sh.lg[r * cp + c2] * rs - (c2 == y ? 1.f : 0.f)) * coef * inv;
                    if (lane == 0) { sh.row_loss[r] = loss; sh.row_hit[r] = am == y ? 1.f : 0.f; }
                } else if (r < cnt4) {
                    for (int c2 = lane; c2 < C; c2 += 16) sh.lg[r * cp + c2] = 0.f;        // a row past the tile's end adds nothing below
                }
            }
            __syncthreads();
            if (t == 0)
                for (int r = 0; r < cnt; ++r) { loss_sum += (double)sh.row_loss[r]; hit_sum += (double)sh.row_hit[r]; }
            // dW and db of this thread's elements
            for (int r0 = 0; r0 < cnt4; r0 += RG) {
                float d[RG];
#pragma unroll
                for (int j = 0; j < RG; ++j) d[j] = sh.lg[(r0 + j) * cp + c];
#pragma unroll
                for (int j = 0; j < RG; ++j) accb += d[j];
#pragma unroll
                for (int k = 0; k < EPT; ++k) {
                    const int e = eg + k * es;
                    const bool on = e < E;
#pragma unroll
                    for (int j = 0; j < RG; ++j) {
                        const float xv = xs[(r0 + j) * E + (on ? e : 0)];
                        acc[k] = fmaf(on ? xv : 0.f, d[j], acc[k]);
                    }
                }
            }
            stash(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        // the update, in registers
        if (adam) {
            const double tt = (double)(job.t0 + step + 1);
            const float lr_t = (float)((double)job.lr * sqrt(1.0 - pow((double)job.beta2, tt)) / (1.0 - pow((double)job.beta1, tt)));
            const float b1 = job.beta1, b2 = job.beta2, eps = job.eps;
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < nk) {
                    m[k] = fmaf(b1, m[k], (1.f - b1) * acc[k]);
                    v[k] = fmaf((1.f - b2) * acc[k], acc[k], b2 * v[k]);
                    w[k] = w[k] - lr_t * m[k] / (sqrtf(v[k]) + eps);
                }
            if (own_bias) {
                mb = fmaf(b1, mb, (1.f - b1) * accb);
                vb = fmaf((1.f - b2) * accb, accb, b2 * vb);
                wb = wb - lr_t * mb / (sqrtf(vb) + eps);
            }
        } else if (job.momentum > 0.f) {
            const float mom = job.momentum, lr = job.lr;
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < nk) {
                    m[k] = mom * m[k] - lr * acc[k];
                    w[k] = w[k] + m[k];
                }
            if (own_bias) { mb = mom * mb - lr * accb; wb = wb + mb; }
        } else {
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < nk) w[k] = fmaf(-job.lr, acc[k], w[k]);
            if (own_bias) wb = fmaf(-job.lr, accb, wb);
        }
        // read behind the barrier that follows the next tile's partial sums
        if (own_bias) sh.bias[t] = wb;
    }

    const bool keep_m = mj && (adam || job.momentum > 0.f), keep_v = vj && adam;
#pragma unroll
    for (int k = 0; k < EPT; ++k)
        if (k < nk) {
            const long i = (long)(eg + k * es) * C + c;
            wj[i] = w[k];
            if (keep_m) mj[i] = m[k];
            if (keep_v) vj[i] = v[k];
        }
    if (own_bias) {
        wj[(long)E * C + t] = wb;
        if (keep_m) mj[(long)E * C + t] = mb;
        if (keep_v) vj[(long)E * C + t] = vb;
    }
    if (t == 0) { stats[2 * (long)blockIdx.x] = (float)loss_sum; stats[2 * (long)blockIdx.x + 1] = (float)hit_sum; }
}

template <int EPT>
int launch_head_fit(const float *emb, const int32_t *labels, int E, const int32_t *order, const float *class_w, const kws_head_job *jobs_dev,
                    int J, float *weights, float *slot_m, float *slot_v, float *stats, hipStream_t s)
{
    KWS_LAUNCH("head_fit_kernel", head_fit_kernel<EPT>, dim3((unsigned)J), dim3(kHfThreads), 0, s, emb, labels, E, order, class_w, jobs_dev, weights,
               slot_m, slot_v, stats);
    KWS_LAUNCH_CHECK("head_fit_kernel");
    return KWS_OK;
}

}  // namespace

}  // namespace kws

using namespace kws;

extern "C" {

int kws_head_fit_max_classes(int E)
{
    if (E < 4 || E > kHfMaxE || E % 4) return 0;
    // registers: E * CP / 256 elements per thread and array, at most kHfMaxEpt; CP a power of two, one column per thread at most
    int cp = 2;
    while (cp * 2 <= kHfMaxCp && (long)E * cp * 2 <= (long)kHfMaxEpt * kHfThreads) cp *= 2;
    // LDS: the block's tiles within the 160 KiB of a CU
    while (cp > 2 && hf_lds_bytes(E, cp) > (size_t)kLdsPerCu) cp /= 2;
    return cp;
}

int kws_head_fit(const float *emb, const int32_t *labels, int64_t N, int E, const int32_t *order, const float *class_weights,
                 const kws_head_job *jobs, void *jobs_dev, int J, float *weights, float *slot_m, float *slot_v, float *stats, void *stream)
{
    if (J < 1) return fail(KWS_ERR_INVALID, "head fit: J = %d jobs (at least 1)", J);
    if (E < 4 || E > kHfMaxE || E % 4) return fail(KWS_ERR_INVALID, "head fit: E = %d is not a multiple of 4 in 4 .. %d", E, kHfMaxE);
    if (N < 1) return fail(KWS_ERR_INVALID, "head fit: N = %lld rows", (long long)N);
    if (!emb || !labels || !order || !jobs || !jobs_dev || !weights || !stats) return fail(KWS_ERR_INVALID, "head fit: null argument");
    if (reinterpret_cast<uintptr_t>(emb) & 15) return fail(KWS_ERR_INVALID, "head fit: emb must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(jobs_dev) & 7) return fail(KWS_ERR_INVALID, "head fit: jobs_dev must be 8-byte aligned");
    const int limit = kws_head_fit_max_classes(E);
    int ept = 1;
    for (int j = 0; j < J; ++j) {
        const kws_head_job &b = jobs[j];
        if (b.batch < 1) return fail(KWS_ERR_INVALID, "head fit: job %d: batch = %d", j, b.batch);
        if (b.num_classes < 2) return fail(KWS_ERR_INVALID, "head fit: job %d: num_classes = %d (at least 2)", j, b.num_classes);
        if (b.n_order < 0 || b.order_offset < 0 || b.weight_offset < 0 || b.t0 < 0)
            return fail(KWS_ERR_INVALID, "head fit: job %d: negative n_order, offset or t0", j);
        if (b.class_weight_offset >= 0 && !class_weights) return fail(KWS_ERR_INVALID, "head fit: job %d names class weights, the array is null", j);
        if (b.optimizer != KWS_OPT_ADAM && b.optimizer != KWS_OPT_SGD)
            return fail(KWS_ERR_UNSUPPORTED, "head fit: job %d: optimizer %d (KWS_OPT_ADAM and KWS_OPT_SGD are built)", j, b.optimizer);
        if (b.optimizer == KWS_OPT_SGD && !(b.momentum >= 0.f && b.momentum <= 1.f))
            return fail(KWS_ERR_INVALID, "head fit: job %d: momentum must be in [0, 1]", j);
        if (b.num_classes > limit)
            return fail(KWS_ERR_UNSUPPORTED, "head fit: job %d: %d classes, at most %d at E = %d (kws_head_fit_max_classes)", j, b.num_classes, limit, E);
        const int per = (int)(((long)E * next_pow2(b.num_classes) + kHfThreads - 1) / kHfThreads);
        ept = std::max(ept, next_pow2(per));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    kws_head_job *jd = static_cast<kws_head_job *>(jobs_dev);
    KWS_HIP_CHECK(hipMemcpyAsync(jd, jobs, sizeof(kws_head_job) * (size_t)J, hipMemcpyHostToDevice, s));
    switch (ept) {
    case 1: return launch_head_fit<1>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    case 2: return launch_head_fit<2>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    case 4: return launch_head_fit<4>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    case 8: return launch_head_fit<8>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    case 16: return launch_head_fit<16>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    default: return launch_head_fit<32>(emb, labels, E, order, class_weights, jd, J, weights, slot_m, slot_v, stats, s);
    }
}

}  // extern "C"
