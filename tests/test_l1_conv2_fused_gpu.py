"""The fused layer-1 + conv2 forward train kernel (csrc/kws_l1_conv2.h: l1_conv2_fwd_bf16_kernel) against the two kernels it replaces.

Default (non-deterministic) training at the default 30 x 20 map runs the fused kernel; deterministic mode keeps
l1m_act_pool_moments_kernel<true> + conv_fwd_clip_bf16_kernel<true>.  Both use the same helpers in the same order, so a1, z2 and
BatchNorm 1's coefficients and moving statistics must agree bit for bit; BatchNorm 2's statistics come from double sums whose
atomic order differs, so they agree to float rounding."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 6
FUSED, L1_OLD, CONV2_OLD = "l1_conv2_fwd_bf16<30,20>", "l1m_act_pool_kernel", "conv_fwd_clip_bf16<16,32>"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def carve(B):
    """float offsets of the workspace arrays this test reads (the head of carve_cnn in csrc/kws_model.hip, simple_cnn, default map)"""
    al = lambda x: (x + 255) & ~255
    off, out = 0, {}

    def take(name, n):
        nonlocal off
        out[name] = (off // 4, n)
        off = al(off + n * 4)
    zs = [0, 15 * 10 * 32, 4 * 3 * 64, 4 * 3 * 128]
    as_ = [15 * 10 * 16, 7 * 5 * 32, 4 * 3 * 64, 256]
    for i in range(4):
        take("z%d" % i, zs[i] * B)
        take("a%d" % i, as_[i] * B)
    for i in range(4):
        take("dwo%d" % i, 0)
    take("d1", B * 128)
    take("loss_i", B)
    take("correct_i", B)
    for i in range(4):
        take("coef%d" % i, 6 * 128)
    return out


def run_step(torch, B, deterministic, prof=False):
    from kws_amd import lib as L
    from kws_amd.init import init_weights
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", C, 30, 20)
    dm = DeviceModel(spec)
    dm.set_weights(init_weights(spec, seed=3))
    dm.set_deterministic(deterministic)
    rng = np.random.default_rng(B)
    x = rng.standard_normal((B, 30, 20)) * 3.0
    x[..., 0] -= 10.0
    feat = torch.from_numpy(x.astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, C, B).astype(np.int32)).cuda()
    if prof:
        L.prof_enable(True)
    try:
        dm.train_fwd_bwd(feat, labels, dropout_seed=11)
        torch.cuda.synchronize()
        report = L.prof_report() if prof else None
    finally:
        if prof:
            L.prof_enable(False)
    lay = carve(B)
    base, _ = dm._workspace(B, True)
    o, nf = base - dm._ws.data_ptr(), max(a + n for a, n in lay.values())
    raw = dm._ws[o:o + 4 * nf].cpu().numpy().view(np.float32)
    get = lambda name: raw[lay[name][0]:lay[name][0] + lay[name][1]].copy()
    bn_state = [t for t in spec.tensors if not t["trainable"]]
    bn_state.sort(key=lambda t: t["offset"])
    state = dm.state.cpu().numpy()
    st = lambda t: state[t["offset"]:t["offset"] + t["size"]].copy()
    return {"a1": get("a0"), "z2": get("z1"), "coef1": get("coef0")[:4 * 16], "coef2": get("coef1")[:4 * 32],
            "mm1": st(bn_state[0]), "mv1": st(bn_state[1]), "mm2": st(bn_state[2]), "mv2": st(bn_state[3])}, report


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("B", [1, 3, 17, 193, 4096])
def test_fused_matches_two_kernel_path(torch, B):
    got, rep = run_step(torch, B, deterministic=False, prof=True)
    want, rep_det = run_step(torch, B, deterministic=True, prof=True)
    assert FUSED in rep and L1_OLD not in rep and CONV2_OLD not in rep, sorted(rep)
    assert FUSED not in rep_det and L1_OLD in rep_det and CONV2_OLD in rep_det, sorted(rep_det)
    for name in ("a1", "z2", "coef1", "mm1", "mv1"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    assert np.isfinite(got["z2"]).all() and np.abs(got["z2"]).max() > 0
    # BatchNorm 2: scale, shift, mean, inv and the moving statistics from double sums (atomic order in default mode)
    for name in ("coef2", "mm2", "mv2"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-6, atol=1e-7, err_msg=name)
    z2 = got["z2"].reshape(B * 150, 32).astype(np.float64)
    np.testing.assert_allclose(got["coef2"][64:96], z2.mean(axis=0), rtol=1e-5, atol=1e-6)
