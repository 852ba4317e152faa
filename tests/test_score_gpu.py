"""GPU tests of kws_score_hist (csrc/kws_score.hip) and of what is built on it (kws_amd.metrics.ScoreStats, KWSModel.evaluate_scores,
eval.py --curves) at the batch, class, bin, score and label edges of the kernel.  Every comparison with tests/score_ref.py is exact
integer equality: there is no tolerance anywhere in this file."""
import os
import re

import numpy as np
import pytest

import score_ref

pytestmark = pytest.mark.gpu

WAVES, UNROLL = 16, 4            # csrc/kws_score.hip: waves of a block, row groups a wave loads before it counts


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def uses_lds(C, bins):
    from kws_amd.metrics import uses_lds as f
    return f(C, bins)


def scores(rng, B, C):
    """softmax-like rows with exact ties, zeros and ones among them"""
    p = rng.dirichlet(np.full(C, 0.4), B).astype(np.float32) if B else np.zeros((0, C), np.float32)
    if B > 4:
        p[B // 2] = p[B // 2, 0]                          # a row of equal scores
        p[B // 3, : min(C, 3)] = p[B // 3, 0]             # a tie among the first classes
        p[1] = 0.0
        p[1, C - 1] = 1.0
    return p


def device_counts(torch, p, y, bins, out=None, rank=True, calib=True):
    """one kws_score_hist call -> the (accumulated) device tensors"""
    from kws_amd import lib as l
    B, C = p.shape
    pd = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda() if B else torch.ones((1, C), device="cuda")    # B == 0: real pointers
    yd = torch.from_numpy(np.ascontiguousarray(y, np.int32)).cuda() if B else torch.zeros((1,), dtype=torch.int32, device="cuda")
    if out is None:
        out = (torch.zeros((C, 2, bins), dtype=torch.int64, device="cuda"), torch.zeros((C,), dtype=torch.int64, device="cuda"),
               torch.zeros((2, bins), dtype=torch.int64, device="cuda"))
    l.check(l.get_lib().kws_score_hist(pd.data_ptr(), yd.data_ptr(), B, C, bins, out[0].data_ptr(), out[1].data_ptr() if rank else None,
                                       out[2].data_ptr() if calib else None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


def check(torch, p, y, bins):
    got = device_counts(torch, p, y, bins)
    want = score_ref.score_counts(p, y, bins)
    for g, w, name in zip(got, want, ("hist", "rank_counts", "calib")):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    return want


# ---- B --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1024, 16384])             # 12 classes: LDS counters / global atomics
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 257])
def test_batch_edges(torch, B, bins):
    C = 12
    assert uses_lds(C, bins) == (bins == 1024)
    rng = np.random.default_rng(B)
    p, y = scores(rng, B, C), rng.integers(0, C, B)
    if B == 0:                                              # a no-op: the outputs keep what they held
        out = tuple(torch.full(s, 7, dtype=torch.int64, device="cuda") for s in [(C, 2, bins), (C,), (2, bins)])
        device_counts(torch, p, y, bins, out=out)
        assert all(bool((o == 7).all()) for o in out)
        return
    want = check(torch, p, y, bins)
    assert want[1].sum() == B and want[0].sum() == B * C


@pytest.mark.parametrize("bins", [16, 8192])
def test_batch_past_one_sweep_of_the_grid(torch, bins):
    """C = 2: 32 rows per wave and group, so one sweep of a full grid covers CUs * 16 * 4 * 32 rows; the batch needs a second, partial
    sweep (the grid stride) whose last group is partial too (the tail)."""
    C = 2
    assert uses_lds(C, bins) == (bins == 16)
    sweep = torch.cuda.get_device_properties(0).multi_processor_count * WAVES * UNROLL * 32
    B = sweep + 5 * WAVES * 32 + 13
    rng = np.random.default_rng(bins)
    a = rng.random(B, dtype=np.float32)
    p = np.stack([a, np.float32(1) - a], 1)
    y = rng.integers(-1, C + 1, B)
    y[-1] = 1                                               # the very last row counts
    check(torch, p, y, bins)


# ---- C and bins -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [8, 2048])
@pytest.mark.parametrize("C", [2, 3, 12, 64, 65, 1024])
def test_class_edges(torch, C, bins):
    rng = np.random.default_rng(C)
    B = 257
    p, y = scores(rng, B, C), rng.integers(0, C, B)
    y[:4] = [0, C - 1, C - 1, 0]
    check(torch, p, y, bins)


BIN_SHAPES = [(2, 2), (2, 1024), (2, 65536), (2, 98304 // 16), (2, 98304 // 16 + 1), (12, 1024), (13, 1024)]


@pytest.mark.parametrize("C,bins", BIN_SHAPES)
def test_bin_edges_and_both_sides_of_the_lds_budget(torch, C, bins):
    rng = np.random.default_rng(bins)
    p, y = scores(rng, 300, C), rng.integers(0, C, 300)
    p[2, 0] = np.nextafter(np.float32(1), np.float32(2))
    check(torch, p, y, bins)


def test_both_counting_paths_are_parametrized():
    budget = int(re.search(r"#define\s+KWS_SCORE_LDS_BUDGET\s+(\d+)", open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include", "kws.h")).read()).group(1))
    assert budget == 98304                                  # BIN_SHAPES names the shapes on either side of it
    paths = {s: uses_lds(*s) for s in BIN_SHAPES}
    assert paths[(2, budget // 16)] and not paths[(2, budget // 16 + 1)] and paths[(12, 1024)] and not paths[(13, 1024)]
    assert paths[(2, 2)] and not paths[(2, 65536)]
    assert {uses_lds(C, b) for C in (2, 3, 12, 64, 65, 1024) for b in (8, 2048)} == {True, False}


# ---- scores on the edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,bins", [(4, 1024), (4, 16384), (2, 2), (70, 64)])
def test_scores_on_the_bin_edges(torch, C, bins):
    """0, 1, the float above 1, every j / bins (exact in fp32) and the float just below it, a negative and a NaN, each as the score of
    every class in turn, under every label"""
    one = np.float32(1)
    grid = np.arange(bins, dtype=np.float32) / np.float32(bins)
    specials = np.concatenate([[np.float32(0), one, np.nextafter(one, np.float32(2)), np.float32(-0.25), np.float32(np.nan)],
                               grid, np.nextafter(grid[1:], np.float32(0))]).astype(np.float32)
    if len(specials) > 600:                                 # the ends of the grid and a stride through its middle
        specials = np.concatenate([specials[:40], specials[40:-40:53], specials[-40:]])
    n = len(specials)
    rng = np.random.default_rng(0)
    p = rng.dirichlet(np.ones(C), n * 2).astype(np.float32)
    cols = np.arange(2 * n) % C
    p[np.arange(2 * n), cols] = np.tile(specials, 2)
    y = np.concatenate([cols[:n], (cols[n:] + 1) % C])      # the special score as target, then as non-target
    want = check(torch, p, y, bins)
    assert want[1][C - 1] >= 2                              # the NaN rows sit at the last rank


@pytest.mark.parametrize("C,bins", [(4, 1024), (4, 16384), (64, 2048), (130, 8)])
def test_all_equal_rows_land_in_one_counter(torch, C, bins):
    """every row the same constant, every label the same class: the rank is the label's index, and each class has ONE live counter that
    all waves of the grid add to -- the worst case for same-address atomics, in LDS and in global memory"""
    B, y0 = 20000, C - 2
    p = np.full((B, C), np.float32(1.0 / C), np.float32)
    y = np.full((B,), y0)
    hist, rank_counts, calib = check(torch, p, y, bins)
    b = int(score_ref.score_bin(np.float32(1.0 / C), bins))
    assert rank_counts[y0] == B and rank_counts.sum() == B
    assert hist[y0, 1, b] == B and all(hist[c, 0, b] == B for c in range(C) if c != y0) and hist.sum() == B * C
    assert calib[0, b] == B and calib[1].sum() == 0


# ---- labels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,bins", [(12, 1024), (12, 16384), (100, 8)])
def test_labels_outside_the_classes_are_skipped(torch, C, bins):
    rng = np.random.default_rng(5)
    B = 700
    p = scores(rng, B, C)
    y = rng.integers(0, C, B)
    y[::3], y[1::7], y[2::11] = -1, C, C + 5
    skipped = int(((y < 0) | (y >= C)).sum())
    want = check(torch, p, y, bins)
    assert skipped > 200 and want[1].sum() == B - skipped and want[2][0].sum() == B - skipped and want[0].sum() == (B - skipped) * C
    none = check(torch, p, np.full((B,), -1), bins)          # nothing counts at all
    assert all(w.sum() == 0 for w in none)
    same = check(torch, p, np.full((B,), 3), bins)           # every label the same class
    assert same[0][3, 0].sum() == 0 and same[0][3, 1].sum() == B


# ---- accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,bins", [(12, 1024), (12, 16384)])
def test_outputs_accumulate_and_optional_outputs_may_be_null(torch, C, bins):
    rng = np.random.default_rng(11)
    B = 1000
    p, y = scores(rng, B, C), rng.integers(-1, C, B)
    want = score_ref.score_counts(p, y, bins)
    out = device_counts(torch, p, y, bins)
    out = device_counts(torch, p, y, bins, out=out)           # the same batch again: every count doubles
    for g, w in zip(out, want):
        np.testing.assert_array_equal(g.cpu().numpy(), 2 * w)
    parts = None
    for lo, hi in [(0, 1), (1, 640), (640, B)]:              # one batch in three calls
        parts = device_counts(torch, p[lo:hi], y[lo:hi], bins, out=parts)
    for g, w in zip(parts, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    only = device_counts(torch, p, y, bins, rank=False, calib=False)
    np.testing.assert_array_equal(only[0].cpu().numpy(), want[0])
    assert int(only[1].sum()) == 0 and int(only[2].sum()) == 0


def test_score_stats_update_merge_counts(torch):
    from kws_amd.metrics import ScoreStats
    rng = np.random.default_rng(2)
    C, bins = 5, 64
    p, y = scores(rng, 500, C), rng.integers(0, C, 500)
    pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    a, b = ScoreStats(C, bins), ScoreStats(C, bins)
    a.update(pd[:200], yd[:200])
    b.update(pd[200:], yd[200:]).update(pd[:0], yd[:0])
    a.merge(b)
    host = ScoreStats.from_counts(*b.counts())
    want = score_ref.score_counts(p, y, bins)
    for g, w in zip(a.counts(), want):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w)
    for g, w in zip(host.merge(ScoreStats.from_counts(*score_ref.score_counts(p[:200], y[:200], bins))).counts(), want):
        np.testing.assert_array_equal(g, w)
    assert a.top_k(C) == 1.0 and a.top_k(1) == want[1][0] / 500
    for c in range(C):
        assert abs(a.auc()[c] - score_ref.pairwise_auc(want[0][c, 1], want[0][c, 0])) <= 1e-12
    with pytest.raises(ValueError):
        a.update(pd[:, :4], yd)


# ---- model level ----------------------------------------------------------------------------------------------------------------
MODEL_TYPES = ["simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"]


def clips(n, C, seed, audio=False):
    from classifier.params import pr
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n)
    if audio:
        return (0.1 * rng.standard_normal((n, pr.max_samples))).astype(np.float32), y
    return rng.standard_normal((n, pr.n_features, pr.feature_size, 1)).astype(np.float32), y


def model_of(model_type, C):
    from classifier.model import get_model
    from kws_amd.init import init_weights
    m = get_model(model_type, C)
    m.set_weights(init_weights(m.spec, seed=1))
    return m


def check_against_matrix(stats, cm, bins):
    hist, rank_counts, calib = stats.counts()
    total = int(cm.sum())
    assert hist.shape == (cm.shape[0], 2, bins)
    assert rank_counts[0] == np.trace(cm) and rank_counts.sum() == total
    np.testing.assert_array_equal(hist[:, 1].sum(1), cm.sum(1))
    np.testing.assert_array_equal(hist[:, 0].sum(1), total - cm.sum(1))
    assert calib[0].sum() == total and calib[1].sum() == np.trace(cm)


@pytest.mark.parametrize("C", [3, 12])
@pytest.mark.parametrize("model_type", MODEL_TYPES)
def test_evaluate_scores_agrees_with_the_confusion_matrix(torch, model_type, C):
    import eval as kws_eval
    names = ["background"] + ["w%d" % i for i in range(1, C)]
    m = model_of(model_type, C)
    x, y = clips(130, C, 7)
    _, cm = kws_eval.evaluate_accuracy(m, x, y, names, batch_size=64)
    stats = m.evaluate_scores(x, y, batch_size=64, bins=256)
    check_against_matrix(stats, cm, 256)
    probs = m.predict(x, batch_size=64)                     # the same counts from the probabilities the host sees
    for g, w in zip(stats.counts(), score_ref.score_counts(probs, y, 256)):
        np.testing.assert_array_equal(g, w)
    if C == 3:                                              # raw audio in: the featurizer runs per batch
        xa, ya = clips(40, C, 8, audio=True)
        _, cma = kws_eval.evaluate_accuracy(m, xa, ya, names, batch_size=16)
        check_against_matrix(m.evaluate_scores(xa, ya, batch_size=16, bins=1024), cma, 1024)


@pytest.mark.parametrize("model_type", MODEL_TYPES)
def test_evaluate_scores_of_an_int8_model(torch, model_type):
    C = 12
    m = model_of(model_type, C)
    x, y = clips(130, C, 9)
    q = m.quantize(x)
    am = q.predict_classes(x, batch_size=64)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (y, am), 1)
    check_against_matrix(m.evaluate_scores(x, y, batch_size=64, bins=1024, quantized=q), cm, 1024)
    stats = m.evaluate_scores(x, y, batch_size=64, bins=1024, quantized=q.quantized)
    for g, w in zip(stats.counts(), score_ref.score_counts(q.predict(x, batch_size=64), y, 1024)):
        np.testing.assert_array_equal(g, w)


# ---- eval.py --------------------------------------------------------------------------------------------------------------------
def test_eval_main_with_and_without_curves(torch, tmp_path, capsys):
    import eval as kws_eval
    C, n = 4, 90
    names = ["background", "yes", "no", "stop"]
    x, y = clips(n, C, 21)
    for i in range(n):
        d = tmp_path / "features" / names[y[i]]
        d.mkdir(parents=True, exist_ok=True)
        np.save(str(d / ("clip_%03d.npy" % i)), x[i])
    (tmp_path / "classes.txt").write_text("\n".join(names) + "\n")
    m = model_of("simple_cnn", C)
    m.save_weights(str(tmp_path / "w.npz"))
    base = ["--model_type", "simple_cnn", "--weights_path", str(tmp_path / "w.npz"), "--dataset_path", str(tmp_path),
            "--classes_path", str(tmp_path / "classes.txt"), "--batch_size", "32"]
    capsys.readouterr()
    kws_eval.main(base)
    plain = capsys.readouterr().out
    csv = tmp_path / "roc.csv"
    kws_eval.main(base + ["--curves", "--bins", "128", "--top_k", "2", "--max_far", "0.05", "--curves_csv", str(csv), "--int8"])
    full = capsys.readouterr().out

    # without --curves: the parent's format -- the loader's lines, the accuracy line, the matrix, nothing else
    lines = plain.splitlines()
    k = [i for i, s in enumerate(lines) if re.fullmatch(r"\d+ correct out of %d samples, accuracy \d\.\d{4}" % n, s)]
    assert len(k) == 1 and len(lines) == k[0] + 2 + C
    w = 11                                                  # max(8, len("background") + 1)
    assert lines[k[0] + 1] == " " * w + "".join("%*s" % (w, c) for c in names)
    cm = np.array([[int(v) for v in s.split()[1:]] for s in lines[k[0] + 2:]])
    assert cm.shape == (C, C) and cm.sum() == n and [s.split()[0] for s in lines[k[0] + 2:]] == names
    assert "AUC" not in plain and "top-1" not in plain

    # with --curves: the same output first, then the table, top-k and ECE; the int8 table after the int8 matrix
    flines = full.splitlines()
    assert flines[:len(lines)] == lines
    table = flines[len(lines):len(lines) + 1 + C + 2]
    assert table[0].split() == ["class", "targets", "non-targets", "AUC", "EER", "EER", "thr", "miss@0.05", "thr@0.05"]
    from classifier.data import get_dataset
    xs, ys, _, _ = get_dataset(str(tmp_path), names)          # the clips in the order eval.py batches them
    capsys.readouterr()
    stats = m.evaluate_scores(xs, ys, batch_size=32, bins=128)
    auc, (eer, _), (thr, miss) = stats.auc(), stats.eer(), stats.at_far(0.05)
    for c in range(C):
        f = table[1 + c].split()
        assert f[0] == names[c] and int(f[1]) == cm[c].sum() and int(f[2]) == n - cm[c].sum()
        assert f[3] == "%.4f" % auc[c] and f[4] == "%.4f" % eer[c] and f[6] == "%.4f" % miss[c] and f[7] == "%.4f" % thr[c]
    assert table[1 + C] == "top-1 accuracy %.4f  top-2 accuracy %.4f" % (stats.top_k(1), stats.top_k(2))
    assert abs(stats.top_k(1) - np.trace(cm) / n) < 1e-12
    assert table[2 + C] == "ECE %.4f (128 confidence bins)" % stats.ece()[0]
    assert full.count("top-1 accuracy") == 2 and "int8:" in flines
    at = flines.index("int8:")                               # the int8 table: the same columns and its differences from the float model
    assert flines[at + 1].split()[:-2] == table[0].split() and flines[at + 1].split()[-2:] == ["EER-fp32", "miss-fp32"]
    assert [s.split()[:3] for s in flines[at + 2:at + 2 + C]] == [s.split()[:3] for s in table[1:1 + C]]
    rows = csv.read_text().splitlines()
    assert rows[0] == "class,threshold,tpr,fpr" and len(rows) == 1 + 2 * C * 129
    assert rows[1].split(",") == ["background", "0", "1", "1"] and rows[1 + C * 129].startswith("int8:background,0,")


# ---- tools/evaluation/validate_speech_commands.py ---------------------------------------------------------------------------------
def test_validate_speech_commands_prints_the_top_k_of_every_file(torch, tmp_path, capsys):
    import importlib.util
    import wave
    from common.data_utils import get_mfcc_feature
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("validate_speech_commands", os.path.join(
        root, "tf-keras-speech-commands_amd", "tools", "evaluation", "validate_speech_commands.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    names = ["background", "yes", "no", "stop", "go"]
    rng = np.random.default_rng(4)
    (tmp_path / "audio").mkdir()
    for i, n in enumerate([16000, 9000, 21000]):              # a full clip, a short one (padded) and a long one (its head is kept)
        w = wave.open(str(tmp_path / "audio" / ("clip%d.wav" % i)), "wb")
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.clip(3000 * rng.standard_normal(n), -32768, 32767).astype("<i2").tobytes()); w.close()
    (tmp_path / "classes.txt").write_text("\n".join(names) + "\n")
    m = model_of("simple_cnn_lite", len(names))
    m.save_weights(str(tmp_path / "w.npz"))
    capsys.readouterr()
    scores, index = tool.main(["--model_type", "simple_cnn_lite", "--weights_path", str(tmp_path / "w.npz"), "--audio_path",
                               str(tmp_path / "audio"), "--classes_path", str(tmp_path / "classes.txt"), "--top_k", "3", "--loop_count", "2",
                               "--output_path", str(tmp_path / "out")])
    out = capsys.readouterr().out.splitlines()
    assert scores.shape == (3, 3) and index.shape == (3, 3) and sum(s.startswith("Average Inference time: ") for s in out) == 1
    for i in range(3):
        path = str(tmp_path / "audio" / ("clip%d.wav" % i))
        want = m.predict(get_mfcc_feature(path)[None])[0]
        order = np.argsort(-want, kind="stable")[:3]
        assert np.abs(np.sort(want)[::-1][:3] - scores[i]).max() < 1e-5
        if np.all(np.diff(want[np.argsort(-want)][:4]) < -1e-4):   # the ranks are settled: the same classes in the same order
            assert index[i].tolist() == order.tolist()
        lines = ["%s: %.3f" % (names[index[i, k]], scores[i, k]) for k in range(3)]
        assert (tmp_path / "out" / ("clip%d.txt" % i)).read_text() == "".join(s + "\n" for s in lines)
        at = out.index(path)
        assert out[at + 1:at + 4] == lines
