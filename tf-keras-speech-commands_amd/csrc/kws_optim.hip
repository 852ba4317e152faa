// csrc/kws_optim.hip -- the optimizer step with the tf.keras optimizer_v2 options (include/kws.h: kws_optimizer_step,
// kws_optimizer_workspace_bytes, kws_optimizer_plan): gradient clipping by value, per-variable norm and global norm, SGD momentum /
// nesterov, RMSprop momentum / centered, Adam amsgrad.  kws_adam_step / kws_sgd_step / kws_rmsprop_step stay the default path.
//
// The buffers are cut into blocks of at most kOptChunk floats, each inside one segment (variable); the block table is built once on the
// host (kws_optimizer_plan) and lives on the device with one double of scratch per block behind it.  Both kernels use the same table:
//   1. opt_sumsq_kernel (norm clipping only): block b writes partial[b] = sum of the squares of its value-clipped g;
//   2. opt_update_kernel: a block sums the partials it needs -- its own segment's, or all of them for the global norm -- in a fixed
//      order, forms the scale, and updates its float4s.  Every block of a segment runs the same sum, so they agree on the bits.
// No atomics and no arrival ticket: two launches, the same bits from run to run.
//
// Weight averaging (kws_optimizer_args.avg / avg_mode / avg_alpha) rides in opt_update_kernel: the new parameter is still in registers
// when the averaging slot is read, folded and stored, so MovingAverage / SWA / Lookahead cost one more read-modify-write of that pass
// and no launch.  The mode is a template parameter: with KWS_AVG_NONE the slot is not touched and the code is the one without it.
// kws_optimizer_swap exchanges params and the slot over the same block table.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "kws_common.h"

namespace kws {
namespace opt {

constexpr int kOptThreads = 256;
constexpr int kOptChunk = 4 * kOptThreads;      // floats per block: one float4 per thread

struct OptBlock {            // 32 bytes; the table a plan writes
    int64_t begin, end;      // [begin, end) inside one segment, begin a multiple of 4
    int32_t first, count;    // the blocks of this block's segment
    int32_t seg, reserved;
};
static_assert(sizeof(OptBlock) == 32, "OptBlock layout");

enum { kNormNone = 0, kNormVar = 1, kNormGlobal = 2 };

struct OptCoef {
    float lr, lr_t, b1, b2, eps, mom, gs, clipvalue, clipnorm, alpha;
    int flags, n_blocks;
};

inline int64_t table_bytes(int64_t nb) { return (nb * (int64_t)sizeof(OptBlock) + 255) & ~(int64_t)255; }
inline int64_t ws_bytes_for(int64_t nb) { return table_bytes(nb) + nb * (int64_t)sizeof(double); }

// tf.clip_by_value; a NaN stays NaN
__device__ __forceinline__ float clip_value(float g, float cv)
{
    return cv > 0.f ? (g > cv ? cv : (g < -cv ? -cv : g)) : g;
}

// sum over the 256 threads of a block, in a fixed order (xor butterfly per wave, then the 4 waves' sums)
__device__ __forceinline__ double block_sum(double x, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(kOptThreads) void opt_sumsq_kernel(const float *__restrict__ g, const OptBlock *__restrict__ tab,
                                                                 float gs, float clipvalue, double *__restrict__ partial)
{
    __shared__ double sh[4];
    const OptBlock b = tab[blockIdx.x];
    const int64_t i = b.begin + 4 * (int64_t)threadIdx.x;
    double s = 0.0;
    if (i + 3 < b.end) {
        const float4 gv = *reinterpret_cast<const float4 *>(g + i);
        const float *gp = &gv.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double ge = clip_value(gp[e] * gs, clipvalue);
            s += ge * ge;
        }
    } else {
        for (int64_t j = i; j < b.end; ++j) {
            const double ge = clip_value(g[j] * gs, clipvalue);
            s += ge * ge;
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one element of the update; g is the transformed gradient.  Contraction is off and the fused multiply-adds are spelled out, so that the
// default options compute what adam_kernel / sgd_kernel / rmsprop_kernel compile to, bit for bit (tests/test_optim_gpu.py)
template <int KIND>
__device__ __forceinline__ void update_one(float &p, float ge, float &m, float &v, float &vh, float &mg, float &mo, const OptCoef &c)
{
#pragma clang fp contract(off)
    if (KIND == KWS_OPT_ADAM) {
        m = fmaf(c.b1, m, (1.f - c.b1) * ge);
        v = fmaf((1.f - c.b2) * ge, ge, c.b2 * v);
        p = p - c.lr_t * m / (sqrtf((c.flags & KWS_OPT_AMSGRAD) ? (vh = fmaxf(vh, v)) : v) + c.eps);
    } else if (KIND == KWS_OPT_RMSPROP) {
        v = c.b2 * v + (1.f - c.b2) * ge * ge;
        float d = v;
        if (c.flags & KWS_OPT_CENTERED) {
            mg = c.b2 * mg + (1.f - c.b2) * ge;
            d = v - mg * mg;
        }
        if (c.mom > 0.f) {
            mo = c.mom * mo + c.lr * ge / sqrtf(d + c.eps);
            p = p - mo;
        } else {
            p = p - c.lr * ge / (sqrtf(d) + c.eps);
        }
    } else {
        if (c.mom > 0.f) {
            mo = c.mom * mo - c.lr * ge;
            p = p + ((c.flags & KWS_OPT_NESTEROV) ? c.mom * mo - c.lr * ge : mo);
        } else {
            p = fmaf(-c.lr, ge, p);
        }
    }
}

// the averaging slot a against the new parameter p.  BLEND is tfa's moving_average_update form (a -= (a - p) alpha: alpha == 1 gives p
// exactly) and leaves p; SYNC is Lookahead's slow step, which both take.  Contraction off, as in update_one.
template <int AVG>
__device__ __forceinline__ void average_one(float &p, float &a, float alpha)
{
#pragma clang fp contract(off)
    if (AVG == KWS_AVG_BLEND) {
        a = a - (a - p) * alpha;
    } else if (AVG == KWS_AVG_SYNC) {
        a = a + alpha * (p - a);
        p = a;
    }
}

template <int KIND, int NORM, int AVG>
__global__ __launch_bounds__(kOptThreads) void opt_update_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                                 float *__restrict__ v, float *__restrict__ vh, float *__restrict__ mg,
                                                                 float *__restrict__ mo, float *__restrict__ av,
                                                                 const OptBlock *__restrict__ tab, const double *__restrict__ partial,
                                                                 OptCoef c)
{
    const OptBlock b = tab[blockIdx.x];
    float num = 1.f, den = 1.f, scale = 1.f;        // per variable: g*num/den (tf.clip_by_norm); global: g*scale
    if (NORM != kNormNone) {
        __shared__ double sh[4];
        const int first = NORM == kNormVar ? b.first : 0, cnt = NORM == kNormVar ? b.count : c.n_blocks;
        double s = 0.0;
        for (int k = threadIdx.x; k < cnt; k += kOptThreads) s += partial[first + k];
        s = block_sum(s, sh);
        const float sq = (float)s;
        if (NORM == kNormVar) {
            const float nrm = sq > 0.f ? (float)sqrt(s) : sq;           // l2sum > 0 ? sqrt(l2sum) : l2sum
            num = c.clipnorm;
            den = nrm != nrm ? nrm : fmaxf(nrm, c.clipnorm);            // tf.maximum propagates a NaN
        } else {
            const float nrm = (float)sqrt(s);
            scale = c.clipnorm * fminf(1.f / nrm, 1.f / c.clipnorm);
            if (!isfinite(nrm)) scale = __builtin_nanf("");
        }
    }
    const bool need_m = KIND == KWS_OPT_ADAM, need_v = KIND != KWS_OPT_SGD;
    const bool need_vh = KIND == KWS_OPT_ADAM && (c.flags & KWS_OPT_AMSGRAD);
    const bool need_mg = KIND == KWS_OPT_RMSPROP && (c.flags & KWS_OPT_CENTERED);
    const bool need_mo = KIND != KWS_OPT_ADAM && c.mom > 0.f;
    auto xform = [&](float gr) {
        float ge = clip_value(gr * c.gs, c.clipvalue);
        if (NORM == kNormVar) ge = ge * num / den;
        if (NORM == kNormGlobal) ge = ge * scale;
        return ge;
    };
    const int64_t i = b.begin + 4 * (int64_t)threadIdx.x;
    if (i + 3 < b.end) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 pv = *reinterpret_cast<float4 *>(p + i), gv = *reinterpret_cast<const float4 *>(g + i);
        float4 mv = need_m ? *reinterpret_cast<float4 *>(m + i) : z, vv = need_v ? *reinterpret_cast<float4 *>(v + i) : z;
        float4 hv = need_vh ? *reinterpret_cast<float4 *>(vh + i) : z, gm = need_mg ? *reinterpret_cast<float4 *>(mg + i) : z;
        float4 ov = need_mo ? *reinterpret_cast<float4 *>(mo + i) : z;
        float *pp = &pv.x, *gp = &gv.x, *mp = &mv.x, *vp = &vv.x, *hp = &hv.x, *gmp = &gm.x, *op = &ov.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) update_one<KIND>(pp[e], xform(gp[e]), mp[e], vp[e], hp[e], gmp[e], op[e], c);
        if (AVG != KWS_AVG_NONE) {
            float4 av4 = *reinterpret_cast<float4 *>(av + i);
            float *ap = &av4.x;
#pragma unroll
            for (int e = 0; e < 4; ++e) average_one<AVG>(pp[e], ap[e], c.alpha);
            *reinterpret_cast<float4 *>(av + i) = av4;
        }
        *reinterpret_cast<float4 *>(p + i) = pv;
        if (need_m) *reinterpret_cast<float4 *>(m + i) = mv;
        if (need_v) *reinterpret_cast<float4 *>(v + i) = vv;
        if (need_vh) *reinterpret_cast<float4 *>(vh + i) = hv;
        if (need_mg) *reinterpret_cast<float4 *>(mg + i) = gm;
        if (need_mo) *reinterpret_cast<float4 *>(mo + i) = ov;
    } else {
        for (int64_t j = i; j < b.end; ++j) {
            float pe = p[j], me = need_m ? m[j] : 0.f, ve = need_v ? v[j] : 0.f, he = need_vh ? vh[j] : 0.f;
            float ge2 = need_mg ? mg[j] : 0.f, oe = need_mo ? mo[j] : 0.f;
            update_one<KIND>(pe, xform(g[j]), me, ve, he, ge2, oe, c);
            if (AVG != KWS_AVG_NONE) {
                float ae = av[j];
                average_one<AVG>(pe, ae, c.alpha);
                av[j] = ae;
            }
            p[j] = pe;
            if (need_m) m[j] = me;
            if (need_v) v[j] = ve;
            if (need_vh) vh[j] = he;
            if (need_mg) mg[j] = ge2;
            if (need_mo) mo[j] = oe;
        }
    }
}

static int check_segments(const int64_t *offsets, const int64_t *sizes, int n_segments, int64_t *n_blocks)
{
    if (!offsets || !sizes || n_segments < 0) return fail(KWS_ERR_INVALID, "optimizer plan: null segment table or n_segments < 0");
    int64_t nb = 0, end = 0;
    for (int s = 0; s < n_segments; ++s) {
        if (offsets[s] < end || (offsets[s] & 3) || sizes[s] < 1)
            return fail(KWS_ERR_INVALID, "optimizer plan: segment %d (offset %lld, size %lld) must follow the previous one, start at a "
                        "multiple of 4 floats and be non-empty", s, (long long)offsets[s], (long long)sizes[s]);
        end = offsets[s] + sizes[s];
        nb += (sizes[s] + kOptChunk - 1) / kOptChunk;
    }
    if (nb > INT32_MAX / 2) return fail(KWS_ERR_INVALID, "optimizer plan: too many blocks");
    *n_blocks = nb;
    return KWS_OK;
}

// exchanges params and the averaging slot inside the blocks of the table; whole words move, so two calls restore every bit
__global__ __launch_bounds__(kOptThreads) void opt_swap_kernel(float *__restrict__ p, float *__restrict__ av, const OptBlock *__restrict__ tab)
{
    const OptBlock b = tab[blockIdx.x];
    const int64_t i = b.begin + 4 * (int64_t)threadIdx.x;
    if (i + 3 < b.end) {
        const float4 pv = *reinterpret_cast<float4 *>(p + i), a4 = *reinterpret_cast<float4 *>(av + i);
        *reinterpret_cast<float4 *>(p + i) = a4;
        *reinterpret_cast<float4 *>(av + i) = pv;
    } else {
        for (int64_t j = i; j < b.end; ++j) {
            const float pe = p[j], ae = av[j];
            p[j] = ae;
            av[j] = pe;
        }
    }
}

template <int KIND, int NORM>
static int launch_update_avg(const kws_optimizer_args *a, const OptBlock *tab, const double *partial, const OptCoef &c, hipStream_t s)
{
    const dim3 grid(a->n_blocks), block(kOptThreads);
    if (a->avg_mode == KWS_AVG_NONE) {
        KWS_LAUNCH("opt_update_kernel", (opt_update_kernel<KIND, NORM, KWS_AVG_NONE>), grid, block, 0, s, a->params, a->grads, a->m, a->v,
                   a->vhat, a->mg, a->mom, a->avg, tab, partial, c);
    } else if (a->avg_mode == KWS_AVG_BLEND) {
        KWS_LAUNCH("opt_update_kernel", (opt_update_kernel<KIND, NORM, KWS_AVG_BLEND>), grid, block, 0, s, a->params, a->grads, a->m, a->v,
                   a->vhat, a->mg, a->mom, a->avg, tab, partial, c);
    } else {
        KWS_LAUNCH("opt_update_kernel", (opt_update_kernel<KIND, NORM, KWS_AVG_SYNC>), grid, block, 0, s, a->params, a->grads, a->m, a->v,
                   a->vhat, a->mg, a->mom, a->avg, tab, partial, c);
    }
    KWS_LAUNCH_CHECK("opt_update_kernel");
    return KWS_OK;
}

template <int KIND>
static int launch_update(int norm, const kws_optimizer_args *a, const OptBlock *tab, const double *partial, const OptCoef &c, hipStream_t s)
{
    if (norm == kNormNone) return launch_update_avg<KIND, kNormNone>(a, tab, partial, c, s);
    if (norm == kNormVar) return launch_update_avg<KIND, kNormVar>(a, tab, partial, c, s);
    return launch_update_avg<KIND, kNormGlobal>(a, tab, partial, c, s);
}

}  // namespace opt
}  // namespace kws

using namespace kws;
using namespace kws::opt;

extern "C" {

int64_t kws_optimizer_workspace_bytes(const int64_t *offsets, const int64_t *sizes, int n_segments)
{
    int64_t nb = 0;
    const int rc = check_segments(offsets, sizes, n_segments, &nb);
    return rc != KWS_OK ? rc : ws_bytes_for(nb);
}

int kws_optimizer_plan(const int64_t *offsets, const int64_t *sizes, int n_segments, void *host_ws, int64_t ws_bytes,
                       int32_t *n_blocks)
{
    int64_t nb = 0;
    const int rc = check_segments(offsets, sizes, n_segments, &nb);
    if (rc != KWS_OK) return rc;
    if (!host_ws || !n_blocks) return fail(KWS_ERR_INVALID, "optimizer plan: null output");
    if (ws_bytes < ws_bytes_for(nb))
        return fail(KWS_ERR_WORKSPACE, "optimizer plan: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                    (long long)ws_bytes_for(nb));
    std::memset(host_ws, 0, (size_t)ws_bytes_for(nb));
    OptBlock *tab = static_cast<OptBlock *>(host_ws);
    int32_t k = 0;
    for (int s = 0; s < n_segments; ++s) {
        const int32_t first = k, count = (int32_t)((sizes[s] + kOptChunk - 1) / kOptChunk);
        for (int32_t j = 0; j < count; ++j, ++k) {
            OptBlock b;
            b.begin = offsets[s] + (int64_t)j * kOptChunk;
            b.end = b.begin + kOptChunk < offsets[s] + sizes[s] ? b.begin + kOptChunk : offsets[s] + sizes[s];
            b.first = first;
            b.count = count;
            b.seg = s;
            b.reserved = 0;
            tab[k] = b;
        }
    }
    *n_blocks = k;
    return KWS_OK;
}

int kws_optimizer_step(const kws_optimizer_args *a, void *stream)
{
    if (!a) return fail(KWS_ERR_INVALID, "null argument");
    if (a->kind < KWS_OPT_SGD || a->kind > KWS_OPT_ADAM) return fail(KWS_ERR_INVALID, "unknown optimizer kind %d", a->kind);
    if (a->flags & ~(KWS_OPT_NESTEROV | KWS_OPT_CENTERED | KWS_OPT_AMSGRAD)) return fail(KWS_ERR_INVALID, "unknown optimizer flags");
    if (!(a->clipvalue >= 0.f) || !(a->clipnorm >= 0.f) || !(a->global_clipnorm >= 0.f))
        return fail(KWS_ERR_INVALID, "clipvalue / clipnorm / global_clipnorm must be >= 0");
    if (a->clipnorm > 0.f && a->global_clipnorm > 0.f)
        return fail(KWS_ERR_INVALID, "clipnorm and global_clipnorm are exclusive");
    if (!(a->momentum >= 0.f && a->momentum <= 1.f)) return fail(KWS_ERR_INVALID, "momentum must be in [0, 1]");
    if (a->kind == KWS_OPT_ADAM && a->t < 1) return fail(KWS_ERR_INVALID, "the step count t must be >= 1");
    if (a->n_blocks < 0) return fail(KWS_ERR_INVALID, "n_blocks < 0");
    if (a->avg_mode < KWS_AVG_NONE || a->avg_mode > KWS_AVG_SYNC) return fail(KWS_ERR_INVALID, "unknown averaging mode %d", a->avg_mode);
    if (a->avg_mode != KWS_AVG_NONE) {
        if (!a->avg) return fail(KWS_ERR_INVALID, "avg_mode %d needs the averaging slot, avg is NULL", a->avg_mode);
        if (reinterpret_cast<uintptr_t>(a->avg) & 15) return fail(KWS_ERR_INVALID, "the averaging slot must be 16-byte aligned");
    }
    if (!(a->avg_alpha >= 0.f && a->avg_alpha <= 1.f)) return fail(KWS_ERR_INVALID, "avg_alpha must be in [0, 1]");
    if (a->n_blocks == 0) return KWS_OK;
    const bool adam = a->kind == KWS_OPT_ADAM, rms = a->kind == KWS_OPT_RMSPROP;
    const bool mom = !adam && a->momentum > 0.f;
    const void *need[] = {a->params, a->grads, adam ? a->m : a->params, (adam || rms) ? a->v : a->params,
                          adam && (a->flags & KWS_OPT_AMSGRAD) ? a->vhat : a->params,
                          rms && (a->flags & KWS_OPT_CENTERED) ? a->mg : a->params, mom ? a->mom : a->params, a->ws};
    for (const void *q : need) {
        if (!q) return fail(KWS_ERR_INVALID, "a buffer this optimizer needs is NULL");
        if (reinterpret_cast<uintptr_t>(q) & 15) return fail(KWS_ERR_INVALID, "optimizer buffers must be 16-byte aligned");
    }
    if (a->ws_bytes < ws_bytes_for(a->n_blocks))
        return fail(KWS_ERR_WORKSPACE, "optimizer workspace of %lld bytes, %lld needed for %d blocks", (long long)a->ws_bytes,
                    (long long)ws_bytes_for(a->n_blocks), a->n_blocks);
    const OptBlock *tab = static_cast<const OptBlock *>(a->ws);
    double *partial = reinterpret_cast<double *>(static_cast<char *>(a->ws) + table_bytes(a->n_blocks));
    const int norm = a->clipnorm > 0.f ? kNormVar : (a->global_clipnorm > 0.f ? kNormGlobal : kNormNone);
    OptCoef c;
    c.lr = a->lr;
    c.lr_t = adam ? (float)((double)a->lr * std::sqrt(1.0 - std::pow((double)a->beta2, (double)a->t)) /
                            (1.0 - std::pow((double)a->beta1, (double)a->t)))
                  : a->lr;
    c.b1 = a->beta1;
    c.b2 = a->beta2;
    c.eps = a->eps;
    c.mom = adam ? 0.f : a->momentum;
    c.gs = a->grad_scale;
    c.clipvalue = a->clipvalue;
    c.clipnorm = norm == kNormVar ? a->clipnorm : a->global_clipnorm;
    c.alpha = a->avg_alpha;
    c.flags = a->flags;
    c.n_blocks = a->n_blocks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (norm != kNormNone) {
        KWS_LAUNCH("opt_sumsq_kernel", opt_sumsq_kernel, dim3(a->n_blocks), dim3(kOptThreads), 0, s, a->grads, tab, c.gs, c.clipvalue,
                   partial);
        KWS_LAUNCH_CHECK("opt_sumsq_kernel");
    }
    if (adam) return launch_update<KWS_OPT_ADAM>(norm, a, tab, partial, c, s);
    if (rms) return launch_update<KWS_OPT_RMSPROP>(norm, a, tab, partial, c, s);
    return launch_update<KWS_OPT_SGD>(norm, a, tab, partial, c, s);
}

int kws_optimizer_swap(float *params, float *avg, const void *ws, int64_t ws_bytes, int32_t n_blocks, void *stream)
{
    if (n_blocks < 0) return fail(KWS_ERR_INVALID, "n_blocks < 0");
    if (!params || !avg || !ws) return fail(KWS_ERR_INVALID, "optimizer swap: null buffer");
    if (params == avg) return fail(KWS_ERR_INVALID, "optimizer swap: params and avg are the same buffer");
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(avg) | reinterpret_cast<uintptr_t>(ws)) & 15)
        return fail(KWS_ERR_INVALID, "optimizer buffers must be 16-byte aligned");
    if (ws_bytes < ws_bytes_for(n_blocks))
        return fail(KWS_ERR_WORKSPACE, "optimizer workspace of %lld bytes, %lld needed for %d blocks", (long long)ws_bytes,
                    (long long)ws_bytes_for(n_blocks), n_blocks);
    if (n_blocks == 0) return KWS_OK;
    KWS_LAUNCH("opt_swap_kernel", opt_swap_kernel, dim3(n_blocks), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), params, avg,
               static_cast<const OptBlock *>(ws));
    KWS_LAUNCH_CHECK("opt_swap_kernel");
    return KWS_OK;
}

}  // extern "C"
