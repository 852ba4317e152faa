// csrc/kws_rnn.hip -- the recurrent models behind the C ABI: 1 .. 4 stacked GRU(48, linear) or LSTM(48, tanh) -> Dense(C, softmax)
// (classifier/models/rnn.py:10-43 and 46-79, classifier/model.py:20-29,37).
#include "kws_gru.h"
#include "kws_lstm.h"
#include "kws_model_types.h"

namespace kws {

namespace {

struct GruWs {
    float *h_last, *loss_i, *correct_i, *saved, *dlogits, *dh_last;
    // stacked models (layer l = 1 .. num_layers - 1): the sequence written by layer l - 1, its saved values, the input gradient it writes
    float *seq[kRnnMaxLayers], *saved_l[kRnnMaxLayers], *dseq[kRnnMaxLayers];
    size_t bytes;
};

size_t saved_floats(const kws_model *m, int B)
{
    return (size_t)B * m->n_features * (m->kind == KWS_SIMPLE_LSTM ? kLstmSave : kGruSave) * kGruU;
}

// the one-layer carve first and unchanged, what the upper layers need behind it
GruWs carve_gru(const kws_model *m, int B, bool training, void *base)
{
    WsCarver c(base);
    GruWs w{};
    w.h_last = c.take((size_t)B * kGruU);
    w.loss_i = c.take(B);
    w.correct_i = c.take(B);
    if (training) {
        w.saved = c.take(saved_floats(m, B));
        w.dlogits = c.take((size_t)B * m->C);
        w.dh_last = c.take((size_t)B * kGruU);
    }
    w.saved_l[0] = w.saved;
    for (int l = 1; l < m->num_layers; ++l) {
        w.seq[l] = c.take((size_t)B * m->n_features * kGruU);
        if (training) {
            w.saved_l[l] = c.take(saved_floats(m, B));
            w.dseq[l] = c.take((size_t)B * m->n_features * kGruU);
        }
    }
    w.bytes = c.off;
    return w;
}

int check(const kws_model *m, int B, bool training, void *ws, size_t ws_bytes, GruWs &w)
{
    if (!ws) return fail(KWS_ERR_INVALID, "null workspace");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(KWS_ERR_INVALID, "workspace must be 256-byte aligned");
    w = carve_gru(m, B, training, ws);
    if (w.bytes > ws_bytes) return fail(KWS_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", w.bytes, ws_bytes);
    return KWS_OK;
}

constexpr size_t kRnnMaxSmem = 160 * 1024;      // the most dynamic LDS a workgroup can opt in to

const char *rnn_name(const kws_model *m) { return m->kind == KWS_SIMPLE_LSTM ? "LSTM" : "GRU"; }

int layer_width(const kws_model *m, int l) { return l == 0 ? m->feature_size : kGruU; }

// Both kernels keep a 16-clip feature tile in LDS, and the backward tile is the larger one: a geometry whose forward kernel fits and
// whose backward kernel does not must be refused BEFORE anything is launched, recorded or called back -- the forward kernel clears the
// caller's gradient buffer.  Every layer of a stacked model is checked here, before the first one runs.
int check_tiles(const kws_model *m, bool training)
{
    for (int l = 0; l < m->num_layers; ++l) {
        const int F = layer_width(m, l);
        const size_t fwd = gru_fwd_smem(m->n_features, F), bwd = gru_bwd_smem(m->n_features, F);
        if (fwd > kRnnMaxSmem)
            return fail(KWS_ERR_UNSUPPORTED, "%s forward tile of %d x %d (layer %d of num_layers = %d) needs %zu B of LDS (limit %zu)",
                        rnn_name(m), m->n_features, F, l, m->num_layers, fwd, kRnnMaxSmem);
        if (training && bwd > kRnnMaxSmem)
            return fail(KWS_ERR_UNSUPPORTED, "%s backward tile of %d x %d (layer %d of num_layers = %d) needs %zu B of LDS (limit %zu)",
                        rnn_name(m), m->n_features, F, l, m->num_layers, bwd, kRnnMaxSmem);
    }
    return KWS_OK;
}

// one layer's view of the step: its input (B, T, F), where its outputs go, its dropout seed
struct LayerIo {
    int l, F;
    const float *in;
    float *h_out, *seq_out, *saved;              // forward: last state (last layer) or whole sequence (the others)
    const float *dh_last, *dseq_in;              // backward: gradient at the last state (last layer) or at every step
    float *dx_out;                               // backward: input gradient (layers >= 1)
    uint64_t seed;
};

LayerIo layer_io(const kws_model *m, int l, const float *feat, const GruWs &w, uint64_t dropout_seed)
{
    const bool last = l == m->num_layers - 1;
    LayerIo io{};
    io.l = l; io.F = layer_width(m, l);
    io.in = l == 0 ? feat : w.seq[l];
    io.h_out = last ? w.h_last : nullptr;
    io.seq_out = last ? nullptr : w.seq[l + 1];
    io.saved = w.saved_l[l];
    io.dh_last = last ? w.dh_last : nullptr;
    io.dseq_in = last ? nullptr : w.dseq[l + 1];
    io.dx_out = l == 0 ? nullptr : w.dseq[l];
    io.seed = KWS_LAYER_DROPOUT_SEED(dropout_seed, l);
    return io;
}

template <typename Kern, typename... Args>
int launch_rnn(const char *name, Kern kern, unsigned threads, size_t smem, int B, hipStream_t s, Args... args)
{
    if (smem > 64 * 1024)
        KWS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    KWS_LAUNCH(name, kern, dim3(blocks_for(B, 16)), dim3(threads), smem, s, args...);
    KWS_LAUNCH_CHECK(name);
    return KWS_OK;
}

template <class Cell, int KX, bool SEQ>
int launch_fwd(const kws_model *m, const LayerIo &io, int B, const float *params, bool save, float rate, hipStream_t s, float *zero_buf,
               long zero_n)
{
    const int T = m->n_features, F = io.F;
    const size_t smem = gru_fwd_smem(T, F);
    const uint32_t slo = (uint32_t)(io.seed & 0xFFFFFFFFu), shi = (uint32_t)(io.seed >> 32);
    if (smem > kRnnMaxSmem) return fail(KWS_ERR_UNSUPPORTED, "%s tile needs %zu B of LDS", rnn_name(m), smem);
    const float *Wk = params + m->o_lk[io.l], *Uk = params + m->o_lu[io.l], *bias = params + m->o_lb[io.l];
    if (save)
        return launch_rnn(Cell::kFwdName, &rnn_fwd_kernel<Cell, KX, true, SEQ>, kGruFwdThreads, smem, B, s, io.in, Wk, Uk, bias, io.h_out, io.saved,
                          B, T, F, rate, slo, shi, zero_buf, zero_n, io.seq_out);
    return launch_rnn(Cell::kFwdName, &rnn_fwd_kernel<Cell, KX, false, SEQ>, kGruFwdThreads, smem, B, s, io.in, Wk, Uk, bias, io.h_out, io.saved, B,
                      T, F, rate, slo, shi, (float *)nullptr, 0L, io.seq_out);
}

template <class Cell, int KX, bool DSEQ, bool DX>
int launch_bwd(const kws_model *m, const LayerIo &io, int B, const float *params, float *grads, float rate, hipStream_t s)
{
    const int T = m->n_features, F = io.F;
    const size_t smem = gru_bwd_smem(T, F);
    const uint32_t slo = (uint32_t)(io.seed & 0xFFFFFFFFu), shi = (uint32_t)(io.seed >> 32);
    if (smem > kRnnMaxSmem) return fail(KWS_ERR_UNSUPPORTED, "%s tile needs %zu B of LDS", rnn_name(m), smem);
    const float *Wk = params + m->o_lk[io.l], *Uk = params + m->o_lu[io.l];
    float *dW = grads + m->o_lk[io.l], *dU = grads + m->o_lu[io.l], *db = grads + m->o_lb[io.l];
    return launch_rnn(Cell::kBwdName, &rnn_bwd_kernel<Cell, KX, DSEQ, DX>, DX ? kGruBwdDxThreads : kGruBwdThreads, smem, B, s, io.in, Uk,
                      (const float *)io.saved, io.dh_last, dW, dU, db, B, T, F, rate, slo, shi, io.dseq_in, Wk, io.dx_out);
}

// Layer 0 takes the template of its width, as the one-layer models always did (their instantiations are SEQ = DSEQ = DX = false); the
// layers above are 48 wide and run the KX = 12 instantiations, the only ones with DX.  launch(KxTag) starts the kernel of that shape.
template <int KX_, bool UPPER_>
struct KxTag {
    static constexpr int KX = KX_;
    static constexpr bool UPPER = UPPER_;
};

template <typename Launch>
int dispatch_kx(const LayerIo &io, Launch launch)
{
    if (io.l > 0) return launch(KxTag<12, true>());
    const int kx = (io.F + 3) / 4;
    if (kx <= 5) return launch(KxTag<5, false>());
    if (kx <= 10) return launch(KxTag<10, false>());
    return launch(KxTag<16, false>());
}

template <class Cell>
int dispatch_fwd(const kws_model *m, const LayerIo &io, int B, const float *params, bool save, float rate, hipStream_t s, float *zero_buf,
                 long zero_n)
{
    return dispatch_kx(io, [&](auto k) {
        return io.seq_out ? launch_fwd<Cell, k.KX, true>(m, io, B, params, save, rate, s, zero_buf, zero_n)
                          : launch_fwd<Cell, k.KX, false>(m, io, B, params, save, rate, s, zero_buf, zero_n);
    });
}

template <class Cell>
int dispatch_bwd(const kws_model *m, const LayerIo &io, int B, const float *params, float *grads, float rate, hipStream_t s)
{
    return dispatch_kx(io, [&](auto k) {
        return io.dseq_in ? launch_bwd<Cell, k.KX, true, k.UPPER>(m, io, B, params, grads, rate, s)
                          : launch_bwd<Cell, k.KX, false, k.UPPER>(m, io, B, params, grads, rate, s);
    });
}

// forward of layers 0 .. N-1 in order; the first one clears zero_buf (the fused-head chain's gradient buffer) when given
int forward_layers(const kws_model *m, const float *feat, int B, const float *params, const GruWs &w, bool save, float rate, uint64_t seed,
                   hipStream_t s, float *zero_buf = nullptr, long zero_n = 0)
{
    for (int l = 0; l < m->num_layers; ++l) {
        const LayerIo io = layer_io(m, l, feat, w, seed);
        float *zb = l == 0 ? zero_buf : nullptr;
        const long zn = l == 0 ? zero_n : 0;
        const int rc = m->kind == KWS_SIMPLE_LSTM ? dispatch_fwd<LstmCell>(m, io, B, params, save, rate, s, zb, zn)
                                                  : dispatch_fwd<GruCell>(m, io, B, params, save, rate, s, zb, zn);
        if (rc) return rc;
    }
    return KWS_OK;
}

// backward of layers N-1 .. 0: each writes the input gradient that the one below adds to its recurrent gradient at every step
int backward_layers(const kws_model *m, const float *feat, int B, const float *params, float *grads, const GruWs &w, float rate, uint64_t seed,
                    hipStream_t s)
{
    for (int l = m->num_layers - 1; l >= 0; --l) {
        const LayerIo io = layer_io(m, l, feat, w, seed);
        const int rc = m->kind == KWS_SIMPLE_LSTM ? dispatch_bwd<LstmCell>(m, io, B, params, grads, rate, s)
                                                  : dispatch_bwd<GruCell>(m, io, B, params, grads, rate, s);
        if (rc) return rc;
    }
    return KWS_OK;
}

}  // namespace

size_t gru_workspace_bytes(const kws_model *m, int B, bool training) { return carve_gru(m, B, training, nullptr).bytes; }

int gru_forward(kws_model *m, const float *feat, int B, const float *params, void *ws, size_t ws_bytes, float *probs,
                int32_t *argmax, hipStream_t s)
{
    GruWs w;
    int rc = check(m, B, false, ws, ws_bytes, w);
    if (rc) return rc;
    rc = check_tiles(m, false);
    if (rc) return rc;
    rc = forward_layers(m, feat, B, params, w, false, 0.f, 0, s);
    if (rc) return rc;
    return run_head(m, B, params, w.h_last, w.loss_i, w.correct_i, nullptr, nullptr, probs, argmax, nullptr, 0.f, nullptr, 0, s);
}

// the inference forward without the head: the last layer's final state (B, 48), copied out of the workspace on the same stream
int gru_embed(kws_model *m, const float *feat, int B, const float *params, void *ws, size_t ws_bytes, float *emb, hipStream_t s)
{
    GruWs w;
    int rc = check(m, B, false, ws, ws_bytes, w);
    if (rc) return rc;
    rc = check_tiles(m, false);
    if (rc) return rc;
    rc = forward_layers(m, feat, B, params, w, false, 0.f, 0, s);
    if (rc) return rc;
    KWS_HIP_CHECK(hipMemcpyAsync(emb, w.h_last, sizeof(float) * (size_t)B * kGruU, hipMemcpyDeviceToDevice, s));
    return KWS_OK;
}

int gru_train_fwd_bwd(kws_model *m, const kws_train_args *a, hipStream_t s)
{
    GruWs w;
    int rc = check(m, a->B, true, a->ws, a->ws_bytes, w);
    if (rc) return rc;
    rc = check_tiles(m, true);
    if (rc) return rc;
    const float rate = a->dropout_seed != 0 ? 0.2f : 0.f;          // GRU / LSTM(dropout=0.2): input dropout, rnn.py:34-35,70-71
    if (head_bwd_fuses(m)) {
        // The first recurrent kernel clears the gradient buffer in its own grid, and the head's forward pass (logits, softmax, loss, dlogits)
        // runs inside its backward kernel (kws_layers.h: head_bwd_mfma_kernel<.., FWD>), as in the simple_cnn step: between the
        // recurrent forward and backward kernels the chain is ONE launch instead of four (head forward, loss sums, memset, head backward)
        rc = forward_layers(m, a->feat, a->B, a->params, w, true, rate, a->dropout_seed, s, a->grads, (long)m->P);
        if (rc) return rc;
        const HeadFwdArgs hf{a->params + m->o_hb, a->labels, a->class_weights, a->probs, w.loss_i, w.correct_i, a->grad_scale / (float)a->B, a->ignore_index};
        rc = run_head_bwd(m, a->B, a->params, w.h_last, nullptr, w.dh_last, a->grads, false, s, nullptr, nullptr, nullptr, nullptr, false, &hf);
        if (rc) return rc;
        if (a->overlap_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->overlap_event), s));
        if (a->overlap_callback) a->overlap_callback(a->overlap_user);
        if (a->forward_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->forward_event), s));
        rc = backward_layers(m, a->feat, a->B, a->params, a->grads, w, rate, a->dropout_seed, s);
        if (rc) return rc;
        if (a->stats) { rc = run_loss_reduce(w.loss_i, w.correct_i, a->B, a->stats, s); if (rc) return rc; }   // fixed-order sums of the per-sample values
        if (a->bucket_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->bucket_event), s));
        return KWS_OK;
    }
    rc = forward_layers(m, a->feat, a->B, a->params, w, true, rate, a->dropout_seed, s);
    if (rc) return rc;
    rc = run_head(m, a->B, a->params, w.h_last, w.loss_i, w.correct_i, a->labels, a->class_weights, a->probs, nullptr, w.dlogits,
                  a->grad_scale / (float)a->B, a->stats, a->ignore_index, s);
    if (rc) return rc;
    if (a->overlap_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->overlap_event), s));
    if (a->overlap_callback) a->overlap_callback(a->overlap_user);
    if (a->forward_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->forward_event), s));
    KWS_HIP_CHECK(hipMemsetAsync(a->grads, 0, sizeof(float) * (size_t)m->P, s));
    rc = run_head_bwd(m, a->B, a->params, w.h_last, w.dlogits, w.dh_last, a->grads, false, s);
    if (rc) return rc;
    rc = backward_layers(m, a->feat, a->B, a->params, a->grads, w, rate, a->dropout_seed, s);
    if (rc) return rc;
    if (a->bucket_event) KWS_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(a->bucket_event), s));
    return KWS_OK;
}

}  // namespace kws
