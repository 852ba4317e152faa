"""GPU tests of the feature-mask stage inside the input pipeline and KWSModel.fit (kws_amd.pipeline.FeaturePipeline.submit(feature_mask=),
KWSModel.fit(feature_mask=)): the pipeline's buffer equals the stand-alone stage and its moments describe the masked features; a mask
that applies to no clip leaves training bit-identical; a mask changes it; pipelined equals stepwise; the dataset, evaluate and
validation never see the mask."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, N, BATCH = 5, 24, 8


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def test_pipeline_masks_its_own_buffer_before_the_moments(torch):
    from kws_amd.augment import FeatureMask
    from kws_amd.model import FeatureMoments
    from kws_amd.pipeline import FeaturePipeline
    rng = np.random.default_rng(0)
    feats = torch.from_numpy(rng.uniform(-60.0, 20.0, (20, 30, 20)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, C, 20).astype(np.int32)).cuda()
    keep = feats.clone()
    fm = FeatureMask(warp=2, rate=0.7, seed=3)
    moments = FeatureMoments(30, 20)
    pipe = FeaturePipeline(None, 8, 30, 20, moments=True, labels=True)
    for step, base, rows in ((5, 16, [3, 19, 0, 7, 7, 12, 1, 4]), (6, 0, [2, 9, 11, 5, 18])):     # a full and a partial batch
        index = torch.tensor(rows, dtype=torch.int32, device="cuda")
        pipe.submit(features=feats, index=index, labels=labels, feature_mask=fm, step=step, position_base=base)
        got, mom, lab = pipe.take()
        gathered = feats.index_select(0, index.long())
        want = fm(gathered, step=step, position_base=base)
        assert torch.equal(_bits(got), _bits(want))
        assert not torch.equal(got, gathered)                  # the mask did change the batch
        assert torch.equal(mom.view(torch.int64), moments(want).view(torch.int64))
        assert not torch.equal(mom, moments(gathered))
        assert torch.equal(lab, labels.index_select(0, index.long()))
        pipe.release()
        torch.cuda.synchronize()
    assert torch.equal(_bits(feats), _bits(keep)), "the source features were written"
    # without index, and without a mask the batch is the source
    pipe.submit(features=feats[:8], labels=labels[:8], feature_mask=fm, step=9)
    got = pipe.take()[0]
    assert torch.equal(_bits(got), _bits(fm(feats[:8].contiguous(), step=9)))
    pipe.release()
    pipe.submit(features=feats[:8], labels=labels[:8])
    assert torch.equal(_bits(pipe.take()[0]), _bits(feats[:8]))
    assert torch.equal(_bits(feats), _bits(keep))


def _fit(torch, model_type, x, y, deterministic, **kw):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    torch.manual_seed(1234)
    m = KWSModel(model_type, C, seed=3)
    if deterministic:
        m._device().set_deterministic(True)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x, y, batch_size=BATCH, epochs=2, verbose=0, shuffle=False, **kw)
    return m, m.get_weights(), h.history["loss"]


def _equal(wa, wb):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(wa, wb))


def test_fit_on_features_with_a_feature_mask(torch):
    from kws_amd.augment import FeatureMask
    rng = np.random.default_rng(5)
    y = rng.integers(0, C, N)
    protos = rng.uniform(-60.0, 20.0, (C, 30, 20))
    x = torch.from_numpy((protos[y] + 2.0 * rng.standard_normal((N, 30, 20))).astype(np.float32)[..., None]).cuda()
    keep = x.clone()
    _, w_plain, loss_plain = _fit(torch, "simple_cnn", x, y, True)
    _, w_off, loss_off = _fit(torch, "simple_cnn", x, y, True, feature_mask=FeatureMask(rate=0.0))
    assert _equal(w_plain, w_off) and loss_plain == loss_off, "a mask that applies to no clip changed the training"
    m, w_on, loss_on = _fit(torch, "simple_cnn", x, y, True, feature_mask=FeatureMask(rate=1.0))
    assert not _equal(w_plain, w_on) and loss_on[0] != loss_plain[0] and loss_on[1] != loss_plain[1]
    _, w_step, loss_step = _fit(torch, "simple_cnn", x, y, True, feature_mask=FeatureMask(rate=1.0), pipeline=False)
    assert _equal(w_on, w_step) and loss_on == loss_step, "pipelined and stepwise training differ under the mask"
    _, w_off_step, _ = _fit(torch, "simple_cnn", x, y, True, feature_mask=FeatureMask(rate=0.0), pipeline=False)
    assert _equal(w_plain, w_off_step)
    assert torch.equal(_bits(x), _bits(keep)), "fit wrote the dataset"
    # evaluate is never masked: the same before and after a mask exists, and the same as a model with these weights that never saw one
    before = m.evaluate(x, y, batch_size=BATCH, verbose=0)
    FeatureMask(rate=1.0)
    assert m.evaluate(x, y, batch_size=BATCH, verbose=0) == before
    from classifier.model import KWSModel
    from classifier.loss import SparseCategoricalCrossEntropy
    from common.model_utils import get_optimizer
    fresh = KWSModel("simple_cnn", C, seed=3)
    fresh._device().set_deterministic(True)
    fresh.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    fresh.set_weights(w_on)
    assert fresh.evaluate(x, y, batch_size=BATCH, verbose=0) == before
    # validation inside fit is not masked either: it is evaluate on the epoch's weights
    m2, _, _ = _fit(torch, "simple_cnn", x, y, True, feature_mask=FeatureMask(rate=1.0), validation_data=(x, y))
    assert [m2.history.history["val_loss"][-1], m2.history.history["val_accuracy"][-1]] == list(m2.evaluate(x, y, batch_size=BATCH, verbose=0))
    assert torch.equal(_bits(x), _bits(keep))


def test_fit_on_raw_audio_with_lengths_and_a_recurrent_model(torch, golden):
    """the eight golden clips twice, with a sample_lengths vector and simple_gru: the recurrent step takes no moments"""
    from kws_amd.augment import FeatureMask
    names = ["right_1", "left_1", "up_1", "down_1", "right_2", "left_2", "up_2", "down_2"]
    pcm = np.stack([golden["pcm_" + n] for n in names] * 2)
    y = np.array([1, 2, 3, 4] * 4)
    lengths = np.array([16000, 12000, 9000, 16000, 15000, 16000, 7000, 14000] * 2, np.int32)
    x = torch.from_numpy(pcm).cuda()
    keep = x.clone()
    _, w_plain, loss_plain = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths)
    _, w_off, loss_off = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths, feature_mask=FeatureMask(rate=0.0))
    assert _equal(w_plain, w_off) and loss_plain == loss_off, "a mask that applies to no clip changed the training"
    _, w_on, loss_on = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths, feature_mask=FeatureMask(rate=1.0))
    assert not _equal(w_plain, w_on) and loss_on[0] != loss_plain[0] and loss_on[1] != loss_plain[1]
    # together with a wave augmentation: the same (step, position) keys, and the mask still decides nothing at rate 0
    from kws_amd.augment import WaveAugment
    aug = WaveAugment(None, loudness=(-30, -15), seed=1)
    _, w_aug, _ = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths, augment=aug)
    _, w_aug_off, _ = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths, augment=aug, feature_mask=FeatureMask(rate=0.0))
    _, w_aug_on, _ = _fit(torch, "simple_gru", x, y, False, sample_lengths=lengths, augment=aug, feature_mask=FeatureMask(rate=1.0))
    assert not _equal(w_plain, w_aug) and _equal(w_aug, w_aug_off) and not _equal(w_aug, w_aug_on)
    # and without lengths or augmentation (the pipeline's plain featurization)
    _, w_bare, _ = _fit(torch, "simple_gru", x, y, False)
    _, w_bare_off, _ = _fit(torch, "simple_gru", x, y, False, feature_mask=FeatureMask(rate=0.0))
    _, w_bare_on, _ = _fit(torch, "simple_gru", x, y, False, feature_mask=FeatureMask(rate=1.0))
    assert _equal(w_bare, w_bare_off) and not _equal(w_bare, w_bare_on)
    assert torch.equal(x, keep)
