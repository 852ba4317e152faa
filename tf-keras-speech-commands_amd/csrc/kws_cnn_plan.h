// csrc/kws_cnn_plan.h -- which kernel form every stage of simple_cnn takes in one call (host only).
//
// plan_cnn() is the ONE place where a path is chosen: kws_model_train_fwd_bwd builds a plan and hands the same object to the forward and the
// backward pass, kws_model_forward / kws_model_prepare_inference build the inference plan; the stage functions in kws_model.hip only read it.
// A flag that follows from another is derived from it, so the two passes cannot disagree about what the forward left for the backward
// (fragment-major weight planes, zmax2 / arg2, the accumulator sets, layer 4's activation).  The builder makes no HIP call: the caller
// queries the stream's capture state once and passes it in.  The shape constants of the kernels it chooses between live in
// kws_cnn_shape.h, the only header this one includes: tests/host/cnn_shape_main.cpp builds plan_cnn with a plain C++ compiler.
#pragma once
#include "kws_cnn_shape.h"

namespace kws {

struct CnnPlan {
    bool training, bf16, det;
    bool prepared;           // inference after kws_model_prepare_inference on the same buffers: the weight planes and BatchNorm coefficients are in place
    bool fused_tail;         // inference with a caller that takes the head's outputs: conv3 .. softmax as one kernel (kws_infer_fused.h)
    bool group;              // conv3 / conv4 forward AND data gradients as clip-group kernels (kws_conv_group.h): fragment-major weight planes
    bool dense_fused;        // Dense forward, head forward / backward and the Dense data gradient as one kernel of the backward pass (kws_dense_head.h)
    bool l1m;                // layer 1 in the MFMA, wave-per-clip forms (kws_layer1.h)
    bool l1_default_map;     // 30 frames x 20 coefficients: the compile-time forms of the layer-1 kernels (kws_layer1_fast.h, kws_l1_conv2.h)
    bool prep_in_stats;      // the weight split and the gradient clear ride in the grid of the layer-1 activation kernel
    bool l1_conv2;           // layer 1 and conv2's forward as ONE clip-resident kernel (kws_l1_conv2.h)
    bool compact_g2;         // conv2's backward keeps g compact: the routed value per pool window + the element index
    bool routed_g2;          // ... and the forward leaves zmax2 / arg2 for the routed reduction (else the index is a byte in da[2])
    bool fuse_pool2;         // conv3's group kernel forms a2 (and zmax2 / arg2) from z2 while it stages its tile
    bool acc_fwd;            // finalize-free batch statistics in the forward pass (kws_device.h: acc_add)
    bool acc_bn2, acc_bn3, acc_bn4;     // ... and in the BatchNorm backward of layers 2, 3, 4
    bool a3_on_load;         // conv4 and its weight gradient form a3 from z3 on the fly (kws_conv.h: ABN / XBN)
    bool pool4_fused;        // layer 4's activation rides in the fused Dense + head kernel of the backward pass (kws_dense_head.h: z4)
    bool wgrad_pmajor;       // conv4's split-precision weight gradient in the position-major form, which skips the padding taps (kws_conv.h: WgradPm)
    bool wgrad2_bf16;        // conv2's weight gradient in split precision
    bool wgrad2_early;       // ... forming dz itself, forked BEFORE conv2's data gradient
    bool wgrad2_fast;        // ... as the wave-per-clip kernel of the default 15 x 10 map (kws_conv2_wgrad_fast.h)
    bool l1_fin_in_kernel;   // layer 1's backward kernel evaluates the closed forms in its last block (no finalize launch)
    bool head_bwd_fuses;     // the MFMA head kernel also leaves the dense bias gradient and the loss / accuracy sums
    bool fuse_head_fwd;      // the head's forward pass rides in its backward kernel
    bool dgrad2_fast;        // conv2's split-precision data gradient as the compile-time kernel of the default 15 x 10 map (kws_conv2_dgrad_fast.h)
};

// what plan_cnn reads of a model (kws_model.hip: cnn_desc)
struct CnnDesc { int kind, C, head_K, deterministic; CnnDims d; };

// mprec: the model's matrix precision (1 = split bf16); capturing: the caller's stream is being captured into a hipGraph;
// wants_head_outputs: an inference caller that takes probs / argmax from the forward itself; prepared: kws_model::prepared_for(...)
inline CnnPlan plan_cnn(const CnnDesc &m, int B, int mprec, bool training, bool capturing, bool wants_head_outputs, bool prepared)
{
    const CnnDims &d = m.d;
    CnnPlan p{};
    p.training = training;
    p.bf16 = mprec == 1;
    p.det = m.deterministic != 0;
    p.prepared = !training && prepared;
    const bool split_train = p.bf16 && training;
    // the geometry the one-kernel inference tail and the clip-group kernels are built for
    const bool default_tail = m.kind == KWS_SIMPLE_CNN && d.H2 == kFuH2 && d.W2 == kFuW2 && d.H3 == kFuH3 && d.W3 == kFuW3;
    p.fused_tail = !training && wants_head_outputs && p.bf16 && default_tail && d.H4 == kFuH4 && d.W4 == kFuW4 && m.C <= kFuHeadCols;
    // the group kernels leave their BatchNorm sums per block: at most kStatStride blocks
    p.group = split_train && default_tail && (long)blocks_for(B, kFuClips) <= kStatStride;
    p.head_bwd_fuses = head_bwd_fuses(m.head_K, m.C);
    p.fuse_head_fwd = p.head_bwd_fuses && !p.det;
    p.dense_fused = split_train && m.kind == KWS_SIMPLE_CNN && p.fuse_head_fwd && m.head_K == kDhK && d.flat % (16 * kDhWaves) == 0 && d.flat <= 1024;
    // every pixel in a pool window, a haloed map of at most 768 floats and at most 40 tiles
    p.l1m = d.H0 % 2 == 0 && d.W0 % 2 == 0 && (d.H0 + 2) * (d.W0 + 2) <= 64 * kL1Stage && (d.H0 / 2) * (d.W0 / 2) <= 4 * kL1MaxTiles;
    p.l1_default_map = d.H0 == 30 && d.W0 == 20;
    p.prep_in_stats = split_train && p.l1m;
    // the clip fits the staging of conv2's kernels
    const int P1 = d.H1 * d.W1;
    p.compact_g2 = p.bf16 && P1 * 8 <= 1280 && (size_t)(d.H1 / 2) * (d.W1 / 2) * 32 <= sizeof(float) * (size_t)d.H3 * d.W3 * 64;
    p.routed_g2 = p.compact_g2;
    p.fuse_pool2 = p.group && p.routed_g2 && d.H1 == kGrH1 && d.W1 == kGrW1;
    // A train step that is being CAPTURED into a hipGraph keeps the partial-sum forms: the accumulator sets' parity and the ticket counter are
    // host-side / device-side state that a replay would not advance (the second replay would add to sums nobody cleared)
    const bool acc_ok = !p.det && !capturing;
    p.acc_fwd = p.fuse_pool2 && acc_ok;
    p.l1_conv2 = p.prep_in_stats && p.acc_fwd && p.l1_default_map;
    // split precision keeps a3 on load; the fp32 mode keeps the activation kernel (same-box A/B at B = 4096: 0.6714 -> 0.666 ms per step)
    p.a3_on_load = split_train;
    p.pool4_fused = p.acc_fwd && p.dense_fused;
    // an output map of at most 16 pixels (the rule of ConvGeom.pmajor); deterministic mode keeps the pixel-major kernel and its single add per element
    p.wgrad_pmajor = split_train && !p.det && d.H3 * d.W3 <= 16;
    p.wgrad2_bf16 = p.bf16 && P1 <= 160;
    // compact g and a clip that fits the kernels' register staging
    p.wgrad2_early = p.compact_g2 && p.wgrad2_bf16 && P1 * 8 <= 1280 && P1 * 4 <= 768;
    // Layer 2: conv3's data gradient does the reduction in its epilogue and conv2's clip kernels derive k2 / k3 from the accumulator set.
    // Layer 3: conv4's data gradient adds its sums to the set and the apply kernel derives the coefficients (needs only the group form, unlike
    // acc_fwd, which needs fuse_pool2).  Layer 4: the fused Dense + head kernel's epilogue is the reduction, the apply kernel expands the compact gradient.
    p.acc_bn2 = p.group && acc_ok && p.routed_g2 && p.wgrad2_early;
    p.acc_bn3 = p.group && acc_ok;
    p.acc_bn4 = p.dense_fused && acc_ok && d.flat == d.H4 * d.W4 * kDhK;
    p.l1_fin_in_kernel = acc_ok && p.l1_default_map;
    // the compile-time map, coefficients from the accumulator set (so neither deterministic mode nor a captured step)
    p.wgrad2_fast = p.wgrad2_early && p.acc_bn2 && d.H1 == kW2fH && d.W1 == kW2fW;
    // the data gradient beside it: same map, same conditions (it takes the place of conv_dgrad_clip_bf16_kernel<true, true, false>)
    p.dgrad2_fast = p.wgrad2_fast;
    return p;
}

}  // namespace kws
