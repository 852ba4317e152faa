"""Case table of the simple_cnn_lite feature-map tests (tests/test_lite_maps_gpu.py, tests/test_lite_maps_host.py).

simple_cnn_lite inference runs two fused kernels whose LDS carve-up, loop bounds and padding come from run-time H, W arguments:
lite_front_infer_kernel (csrc/kws_lite.h: stages 1 and 2, one wave per clip) and lite_back_f16_kernel (csrc/kws_lite_f16.h: a2 to the
probabilities, 16 clips per block).  The rows below are feature maps on both sides of every rule that admits a map to either kernel,
with every placement of the stride-2 'same' padding of depthwise 3, and two batch sizes (computed from the device's compute-unit count)
at which the kernels' clip loops take their second pass with a short remainder.  Everything here is host-only: the restated admission
rules of the library, the oracle models, the inputs and the shared oracle results.

Models are head_cases.float_model: with plain Glorot weights the probabilities are almost uniform and every tolerance hides a wrong
kernel; the centred, scaled head makes many classes win somewhere.  The fp32 comparisons use logits of spread 1.5, the fp16 ones 0.3
(fp16 logit errors grow with the head's scale; tests/test_heads_gpu.py: test_lite_fp16_head_columns).

The arg-max is compared where the oracle's two best classes are further apart than twice the probability tolerance.  That mask is a
condition on the inputs: at most MASK_CAP_FP32 of a case's clips may fall under it in fp32, MASK_CAP_FP16 in fp16.  The seeds were
chosen with the float64 oracle alone so that these caps hold and that swapping the padding side moves the probabilities by more than
MUTATION_FACTOR tolerances (tests/test_lite_maps_host.py asserts both); no seed was chosen by looking at device output."""
import collections

import numpy as np

import head_cases as hc
from cnn_path_cases import MI355X_CUS, dims                    # CnnDims of kws_model_create, shared by both CNN kinds
from oracle import model_oracle as mo

KIND = "simple_cnn_lite"
C, B = 12, 37                                                  # 37 clips: two fp16 tiles and 5 clips
TOL_FP32, GAP_FP32, SPREAD_FP32, MASK_CAP_FP32 = 1e-4, 2e-4, 1.5, 0.05
TOL_FP16, GAP_FP16, SPREAD_FP16, MASK_CAP_FP16 = 1e-3, 2e-3, 0.3, 0.20
MUTATION_FACTOR = 100


# ---- the library's admission rules, restated ----------------------------------------------------------------------------
def pad_before(n, k, s):
    """same_pad_before (csrc/kws_cnn_shape.h): TF 'SAME' puts the odd padding pixel at the end"""
    out = -(-n // s)
    return max((out - 1) * s + k - n, 0) // 2


def front_ok(nf, fs):
    """lite_front_applies (csrc/kws_lite.h): every stage-1 pixel in a pool window, a haloed map of at most 768 floats"""
    d = dims(nf, fs)
    return nf % 2 == 0 and fs % 2 == 0 and (nf + 2) * (fs + 2) <= 64 * 12 and d["H2"] >= 1 and d["W2"] >= 1


def f16_ok(nf, fs, classes=C):
    """LiteCtx::forward_f16 (lite_front_applies and lite_f16_fits, csrc/kws_lite_f16.h): kF16MaxN2 = 35 a2 pixels, kF16MaxP3 = 12 stage-3 pixels, kWdRow = 256 Dense inputs, kF16HeadCols = 48"""
    d = dims(nf, fs)
    return (front_ok(nf, fs) and d["H2"] * d["W2"] <= 35 and d["H3"] * d["W3"] <= 12 and d["H4"] >= 1 and d["W4"] >= 1
            and classes <= 48 and d["flat"] <= 256)


def front_lds_bytes(nf, fs):
    """lite_front_floats (csrc/kws_lite.h): a1 with its halo, then xs + d1 sharing their space with d2"""
    H1, W1 = nf // 2, fs // 2
    n2 = (H1 // 2) * (W1 // 2)
    p2 = 16 * ((n2 + 3) // 4)
    a, b = (nf + 2) * (fs + 2) + nf * fs, p2 * 17
    return 4 * (((H1 + 2) * (W1 + 2) * 16 + max(a, b) + 3) & ~3)


def front_waves(cus, nf=16, fs=16):
    """the waves the front kernel's grid is sized for: up to 8 per compute unit within 160 KiB of LDS; beyond, a wave takes several clips"""
    return cus * max(1, min(8, 160 * 1024 // front_lds_bytes(nf, fs)))


def clips_per_wave(batch, cus, nf=16, fs=16):
    waves = front_waves(cus, nf, fs)
    return max(1, (batch + waves - 1) // waves)


# ---- the maps -------------------------------------------------------------------------------------------------------------
# name, frames, coefficients, then the stated geometry: (H1, W1), (H2, W2), (H3, W3), flat, front kernel?, fp16 kernel?, (pt3, pl3), and
# the seed (module docstring).  tests/test_lite_maps_host.py holds every stated value against the restated rules.
Map = collections.namedtuple("Map", "name nf fs s1 s2 s3 flat front f16 pad3 seed why")
MAPS = (
    Map("30x20", 30, 20, (15, 10), (7, 5), (4, 3), 256, True, True, (1, 1), 3020, "control: the default map, pt3 = pl3 = 1"),
    Map("24x16", 24, 16, (12, 8), (6, 4), (3, 2), 128, True, True, (0, 0), 2416, "pt3 = pl3 = 0; H3 = 3 odd; one pooled pixel"),
    Map("26x14", 26, 14, (13, 7), (6, 3), (3, 2), 128, True, True, (0, 1), 2614, "pt3 = 0, pl3 = 1; H1 = 13 and W1 = 7 odd"),
    Map("22x18", 22, 18, (11, 9), (5, 4), (3, 2), 128, True, True, (1, 0), 2218, "pt3 = 1, pl3 = 0; H1 = 11 and W1 = 9 odd"),
    Map("16x16", 16, 16, (8, 8), (4, 4), (2, 2), 128, True, True, (0, 0), 1616, "smallest accepted; P3 = 4; the batch edges' map"),
    Map("30x12", 30, 12, (15, 6), (7, 3), (4, 2), 256, True, True, (1, 1), 3012, "narrow: W1 = 6, W2 = 3, W3 = 2"),
    Map("22x30", 22, 30, (11, 15), (5, 7), (3, 4), 256, True, True, (1, 1), 2230,
        "(H+2)(W+2) = 768, n2 = 35, P3 = 12, flat = 256: every limit at its edge, the default transposed"),
    Map("12x44", 12, 44, (6, 22), (3, 11), (2, 6), 384, True, False, (1, 1), 1244, "fp16 refused by the Dense row alone (n2 = 33, P3 = 12)"),
    Map("24x26", 24, 26, (12, 13), (6, 6), (3, 3), 128, True, False, (0, 0), 2426, "fp16 refused (n2 = 36, a2 is 6 x 6); pt3 = pl3 = 0"),
    Map("32x20", 32, 20, (16, 10), (8, 5), (4, 3), 256, True, False, (0, 1), 3220, "fp16 refused (n2 = 40); pt3 = 0"),
    Map("24x30", 24, 30, (12, 15), (6, 7), (3, 4), 256, False, False, (0, 1), 2430, "(H+2)(W+2) = 832 > 768: the layer-by-layer path; fp16 refused"),
)
MAP = {m.name: m for m in MAPS}
PREPARED_MAP = "24x16"
EDGE_MAP = "16x16"
EDGES = ("fp32", "fp16")


def edge_batch(path, cus):
    """fp32: one clip more than the front kernel's waves -- two clips per wave, one clip in the last wave.
    fp16: 16 clips per tile and one block per compute unit -- the tile loop's second pass runs, with one clip in the last tile."""
    m = MAP[EDGE_MAP]
    return front_waves(cus, m.nf, m.fs) + 1 if path == "fp32" else 16 * cus + 17


# ---- builders ---------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "om x want clear")
_MODELS, _REFERENCES = {}, {}


def model(m, path):
    """the oracle model of a map for the fp32 (spread 1.5) or fp16 (spread 0.3) comparison; its weights are the device's float32 values"""
    key = (m.name, path)
    if key not in _MODELS:
        fp16 = path == "fp16"
        _MODELS[key] = hc.float_model(KIND, C, seed=m.seed + (10 if fp16 else 0), spread=SPREAD_FP16 if fp16 else SPREAD_FP32,
                                      n_features=m.nf, feature_size=m.fs)
    return _MODELS[key]


def inputs(m, batch):
    """the first clips are the same for every batch size (the generator fills clip by clip)"""
    return hc.features(batch, m.seed + 20, n_features=m.nf, feature_size=m.fs)


def reference(m, path, batch=B):
    """(oracle model, features float32, float64 probabilities, the clips whose arg-max is compared), computed once per (map, path, batch)"""
    key = (m.name, path, batch)
    if key not in _REFERENCES:
        om, x = model(m, path), inputs(m, batch)
        want = om.predict(x.astype(np.float64))
        top2 = np.sort(want, axis=-1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > (GAP_FP16 if path == "fp16" else GAP_FP32)
        for a in (x, want, clear):
            a.setflags(write=False)
        _REFERENCES[key] = Reference(om, x, want, clear)
    return _REFERENCES[key]


def mask_cap(path):
    return MASK_CAP_FP16 if path == "fp16" else MASK_CAP_FP32


def paths(m):
    """the comparisons a map takes part in: fp32 everywhere, fp16 where the library accepts the map"""
    return ("fp32", "fp16") if m.f16 else ("fp32",)


def swapped_padding_probs(om, x):
    """the oracle's probabilities with the odd padding pixel of every stride-2 'same' convolution moved to the front"""
    orig = mo.same_pad

    def swapped(n_in, k, s):
        n_out, before, after = orig(n_in, k, s)
        return (n_out, after, before) if s == 2 else (n_out, before, after)
    mo.same_pad = swapped
    try:
        return om.predict(x.astype(np.float64))
    finally:
        mo.same_pad = orig
