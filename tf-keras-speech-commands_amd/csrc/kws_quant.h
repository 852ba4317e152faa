// csrc/kws_quant.h -- int8 simple_cnn (include/kws.h: kws_model_calibrate, kws_quantize_simple_cnn, kws_qmodel_*): the geometry the
// quantized forward is built for, the fragment-major weight layout its kernel reads and the device-side model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws.h"

namespace kws {
namespace q8 {
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The default geometry: 30 x 20 -> conv1 + pool 15 x 10 x 16 -> conv2 + pool 7 x 5 x 32 -> conv3 (stride 2) 4 x 3 x 64 -> conv4 + pool
// 2 x 1 x 128 -> Dense 128 -> head C.
constexpr int kH0 = 30, kW0 = 20;
constexpr int kC1 = 16, kC2 = 32, kC3 = 64, kC4 = 128, kFlat = 256, kD = 128;
constexpr int kHead = KWS_QUANT_MAX_CLASSES;   // head columns padded to three 16-column tiles

// Fragment-major weights of the matrix layers (v_mfma_i32_16x16x64_i8).  Fragment (s, ct) of a layer with K reduced rows (HWIO
// flattening k = tap * CI + ci) and N columns is 64 lanes x 16 bytes: byte j of lane l = W[k = 64 s + 16 (l >> 4) + j][16 ct + (l & 15)],
// 0 past K or N; stored at ((s * NCT + ct) * 64 + l).  For conv2 (CI = 16) a lane quarter is one tap, for conv3 (CI = 32) half a tap,
// for conv4 (CI = 64) a k-step is one tap: the A side reads the same 16 channels of one haloed input pixel.
constexpr int kS2 = 3, kN2 = 2;     // K = 144 (9 taps x 16, padded to 192)
constexpr int kS3 = 5, kN3 = 4;     // K = 288 (padded to 320)
constexpr int kS4 = 9, kN4 = 8;     // K = 576
constexpr int kSd = 4, kNd = 8;     // K = 256
constexpr int kSh = 2, kNh = 3;     // K = 128, C <= 48
// epilogue constants, one fp32 array: M1 B1 M2 B2 M3 B3 M4 B4 Md Bd Mh head_bias (the order of kws_qsimple_cnn)
constexpr int kEpM1 = 0, kEpB1 = 16, kEpM2 = 32, kEpB2 = 64, kEpM3 = 96, kEpB3 = 160, kEpM4 = 224, kEpB4 = 352;
constexpr int kEpMd = 480, kEpBd = 608, kEpMh = 736, kEpHb = 784, kEpCount = 832;
}  // namespace q8
}  // namespace kws

struct kws_qmodel {
    int C = 0;
    int device = -1;
    float inv_s0 = 0.f;
    void *blob = nullptr;                 // one device allocation holding everything below
    const int32_t *w1 = nullptr;          // conv1: [16][3] int32 = the 9 taps of a channel packed 4 per word (tap 8 alone in the third)
    const kws::q8::i32x4 *f2 = nullptr, *f3 = nullptr, *f4 = nullptr, *fd = nullptr, *fh = nullptr;
    const float *ep = nullptr;            // kEpCount floats
};
