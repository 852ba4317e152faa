"""simple_cnn_lite inference on feature maps other than 30 x 20, against the float64 oracle (oracle/model_oracle.py).

lite_front_infer_kernel (csrc/kws_lite.h) and lite_back_f16_kernel (csrc/kws_lite_f16.h) take their LDS carve-up, loop bounds and
padding from run-time H, W arguments; the rest of the suite reaches them at 30 x 20 only, where a2 is 7 x 5 and the stride-2 'same'
padding of depthwise 3 is symmetric.  tests/lite_map_cases.py holds the maps (every placement of that padding, odd stage-1 and
stage-3 maps, each admission limit at its edge and one step beyond), the restated admission rules and the shared oracle results;
tests/test_lite_maps_host.py proves on the oracle alone that a kernel padding on the wrong side would move the probabilities of the
maps with an even a2 side by more than a hundred tolerances, and that the arg-max masks below stay under their caps.

Bounds (the suite's existing ones for the same quantities) and what this suite measured on an MI355X:
  fp32 probabilities within 1e-4 of the oracle (test_lite_inference_forward, test_other_geometries_train_and_infer): measured
    30x20 8.9e-7, 24x16 9.3e-7, 26x14 1.7e-6, 22x18 6.8e-7, 16x16 9.2e-7, 30x12 1.1e-6, 22x30 7.3e-7, 12x44 1.2e-6, 24x26 9.4e-7,
    32x20 1.2e-6, 24x30 (layer by layer) 8.1e-7; 16x16 at 2049 clips 1.7e-6;
  fp16 probabilities within 1e-3 of the oracle and of the fp32 device path (test_lite_inference_forward_fp16): measured, the same
    against both, 30x20 2.6e-4, 24x16 1.4e-4, 26x14 1.8e-4, 22x18 1.9e-4, 16x16 2.3e-4, 30x12 1.8e-4, 22x30 1.9e-4; 16x16 at 4113
    clips 4.1e-4;
  fp16 rows sum to 1 within 1e-5; the arg-max is exact where the oracle's two best classes are more than twice the tolerance apart.
Every case prints a "FIGURES | map | path | max error" line."""
import numpy as np
import pytest

import head_cases as hc
import lite_map_cases as lc

pytestmark = pytest.mark.gpu

IDS = [m.name for m in lc.MAPS]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def on_device(torch, x):
    return torch.from_numpy(np.array(x)).cuda()             # a copy: the shared reference arrays are read-only


def forward(torch, dm, xt):
    probs, am = dm.forward(xt)
    return probs.cpu().numpy(), am.cpu().numpy()


def profiled_forward(torch, dm, xt):
    """-> (labels of the launches of one forward, its probabilities)"""
    from kws_amd import lib as L
    L.prof_enable(True)
    try:
        probs, _ = dm.forward(xt)
        torch.cuda.synchronize()
        return set(L.prof_report()), probs.cpu().numpy()
    finally:
        L.prof_enable(False)


def check_front_labels(labels, m, what):
    """the fused front kernel exactly where the library admits the map, the layer-by-layer stages 1 and 2 exactly where not"""
    assert ("lite_front_infer_kernel" in labels) == m.front, (what, sorted(labels))
    for per_layer in ("dwconv_fwd_kernel.L1", "dwconv_fwd_kernel.L2"):
        assert (per_layer in labels) == (not m.front), (what, sorted(labels))
    assert {"dwconv_fwd_kernel.L3", "dwconv_fwd_kernel.L4"} <= labels, (what, sorted(labels))


def check_fp32(probs, am, ref, what):
    """fp32 probabilities and class indices of every clip against the oracle's; -> max error"""
    assert probs.shape == ref.want.shape and np.isfinite(probs).all(), what
    assert (~ref.clear).mean() <= lc.MASK_CAP_FP32, what                       # a condition on the inputs (lite_map_cases docstring)
    err = float(np.abs(probs - ref.want).max())
    print("FIGURES | %s | fp32 | %.2e" % (what, err))
    assert err < lc.TOL_FP32, (what, err)
    np.testing.assert_array_equal(am[ref.clear], ref.want.argmax(-1)[ref.clear], err_msg=what)
    return err


def check_fp16(p16, a16, p32, ref, what):
    """fp16 probabilities and class indices of every clip against the oracle's and the fp32 device path's; -> max error"""
    assert p16.shape == ref.want.shape and np.isfinite(p16).all(), what
    assert (~ref.clear).mean() <= lc.MASK_CAP_FP16, what
    err, err32 = float(np.abs(p16 - ref.want).max()), float(np.abs(p16 - p32).max())
    print("FIGURES | %s | fp16 | %.2e (against the fp32 device path %.2e)" % (what, err, err32))
    assert err < lc.TOL_FP16, (what, err)
    assert err32 < lc.TOL_FP16, (what, err32)
    assert err32 > 0, what                                                      # the fp16 path really ran
    np.testing.assert_allclose(p16.sum(-1), 1.0, atol=1e-5, rtol=0, err_msg=what)
    np.testing.assert_array_equal(a16[ref.clear], ref.want.argmax(-1)[ref.clear], err_msg=what)
    return err


@pytest.mark.parametrize("m", lc.MAPS, ids=IDS)
def test_lite_map_fp32_against_the_oracle(torch, m):
    ref = lc.reference(m, "fp32")
    dm = hc.device_model(ref.om)
    assert (dm.spec.n_features, dm.spec.feature_size) == (m.nf, m.fs)
    xt = on_device(torch, ref.x)
    probs, am = forward(torch, dm, xt)
    check_fp32(probs, am, ref, m.name)
    labels, again = profiled_forward(torch, dm, xt)
    check_front_labels(labels, m, m.name)
    assert "lite_back_f16_kernel" not in labels
    np.testing.assert_array_equal(again, probs)


@pytest.mark.parametrize("m", lc.MAPS, ids=IDS)
def test_lite_map_fp16_against_the_oracle_or_refused(torch, m):
    from kws_amd import lib as L
    if not m.f16:
        # refused with KWS_ERR_UNSUPPORTED, never served by another path; the model still answers in fp32 afterwards
        ref = lc.reference(m, "fp32")
        dm = hc.device_model(ref.om)
        xt = on_device(torch, ref.x)
        before, _ = forward(torch, dm, xt)
        dm.set_precision(infer=L.INFER_FP16)
        with pytest.raises(L.KwsError, match="fp16 inference"):
            dm.forward(xt)
        dm.set_precision(infer=L.INFER_FP32)
        probs, am = forward(torch, dm, xt)
        np.testing.assert_array_equal(probs, before)
        check_fp32(probs, am, ref, "%s after the fp16 refusal" % m.name)
        return
    ref = lc.reference(m, "fp16")
    dm = hc.device_model(ref.om)
    xt = on_device(torch, ref.x)
    p32, _ = forward(torch, dm, xt)
    assert float(np.abs(p32 - ref.want).max()) < lc.TOL_FP32                  # the fp32 path on this model too
    dm.set_precision(infer=L.INFER_FP16)
    assert dm.get_precision()[1] == L.INFER_FP16
    p16, a16 = forward(torch, dm, xt)
    check_fp16(p16, a16, p32, ref, m.name)
    labels, again = profiled_forward(torch, dm, xt)
    np.testing.assert_array_equal(again, p16)                                 # a second call: bit-identical
    assert {"lite_front_infer_kernel", "lite_back_f16_kernel"} <= labels, sorted(labels)
    assert not any(l.startswith("dwconv_fwd_kernel") for l in labels), sorted(labels)


def test_prepared_inference_equals_the_unprepared_one_off_the_default_map(torch):
    """kws_model_prepare_inference on 24 x 16 (pt3 = pl3 = 0, flat = 128: the Dense rows of the fp16 blob are half empty): the prepared
    forwards skip the weight-derived launches and give the unprepared forwards' bits"""
    from kws_amd import lib as L
    m = lc.MAP[lc.PREPARED_MAP]
    ref = lc.reference(m, "fp16")
    dm = hc.device_model(ref.om)
    xt = on_device(torch, ref.x)
    for infer, derived in ((L.INFER_FP32, {"bn_infer_coef_all_kernel"}), (L.INFER_FP16, {"bn_infer_coef_all_kernel", "lite_f16_prepare_kernel"})):
        dm.set_precision(infer=infer)
        labels, plain = profiled_forward(torch, dm, xt)
        assert derived <= labels, sorted(labels)
        dm.prepare_inference(lc.B)
        labels, prepared = profiled_forward(torch, dm, xt)
        assert not (labels & {"bn_infer_coef_all_kernel", "lite_f16_prepare_kernel"}) and "lite_front_infer_kernel" in labels, sorted(labels)
        np.testing.assert_array_equal(prepared, plain)
        assert float(np.abs(prepared - ref.want).max()) < (lc.TOL_FP16 if infer == L.INFER_FP16 else lc.TOL_FP32)
        assert ("lite_back_f16_kernel" in labels) == (infer == L.INFER_FP16)


@pytest.mark.parametrize("path", lc.EDGES)
def test_lite_batch_edges_against_the_oracle(torch, path):
    """16 x 16 at the batch sizes (from this device's compute-unit count) where the front kernel's waves take two clips with one clip
    left for the last wave (fp32), and where the fp16 kernel's tile loop runs a second pass with one clip in the last tile; every
    clip is compared"""
    from kws_amd import lib as L
    m = lc.MAP[lc.EDGE_MAP]
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    batch = lc.edge_batch(path, cus)
    ref = lc.reference(m, path, batch)
    dm = hc.device_model(ref.om)
    xt = on_device(torch, ref.x)
    p32, a32 = forward(torch, dm, xt)
    what = "%s B = %d (%d compute units)" % (m.name, batch, cus)
    if path == "fp32":
        assert lc.clips_per_wave(batch, cus) == 2 and batch % 2 == 1
        check_fp32(p32, a32, ref, what)
        labels, again = profiled_forward(torch, dm, xt)
        check_front_labels(labels, m, what)
        np.testing.assert_array_equal(again, p32)
    else:
        assert -(-batch // 16) == cus + 2 and batch % 16 == 1
        assert float(np.abs(p32 - ref.want).max()) < lc.TOL_FP32
        dm.set_precision(infer=L.INFER_FP16)
        p16, a16 = forward(torch, dm, xt)
        check_fp16(p16, a16, p32, ref, what)
        labels, again = profiled_forward(torch, dm, xt)
        np.testing.assert_array_equal(again, p16)
        assert "lite_back_f16_kernel" in labels, sorted(labels)
