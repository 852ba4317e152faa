"""The shape and launch rules of simple_cnn (csrc/kws_cnn_shape.h, csrc/kws_cnn_plan.h) without a device: tests/host/cnn_shape_main.cpp,
built here with the plain C++ compiler, answers queries about every rule, and the answers are held to the Python restatements the GPU
suites rest on (tests/cnn_path_cases.py, tests/wgrad_pmajor_cases.py, tests/lite_train_cases.py, tests/lite_map_cases.py).  Where no
restatement exists (the one-resident-round grids of the weight gradients, the channel reductions' row split, the clip grids) the answers
are held to what the kernels need of their launch: every row covered, no empty last block, the grid within its bound."""
import json
import os
import shutil
import subprocess

import pytest

import cnn_path_cases as cc
import geometry_cases as gc
import lite_map_cases as lm
import lite_train_cases as lt
import wgrad_pmajor_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "cnn_shape_main.cpp")
CHANNELS = (1, 16, 32, 64, 128)                     # kCh
SIMPLE_CNN, HEAD_K = 0, 128                         # KWS_SIMPLE_CNN; the Dense layer in front of simple_cnn's head
PLAN_MODES = ("default", "fp32", "det", "fp32+det")
SWEEP = range(1, 5001)
SLOTS = (1, 7, 768, 2048)
PM_BATCHES = tuple(range(1, 71)) + tuple(range(680, 1401))          # tests/test_wgrad_pmajor_host.py: BATCHES


def _maps():
    maps = [(r.nf, r.fs) for r in cc.ROWS] + list(wc.MAPS) + [(c.nf, c.fs) for c in lt.CASES] + [(m.nf, m.fs) for m in lm.MAPS]
    maps += [(gc.clip_frames(g), gc.feature_size(g)) for g in gc.ROWS]
    return sorted(set(maps))


MAPS = _maps()


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("cnn_shape") / "cnn_shape")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tf-keras-speech-commands_amd", "csrc"), SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and not r.stdout.strip(), "the host program must build without a warning:\n" + r.stdout

    def ask(queries, status=0):
        """one answer (a dict) per query line"""
        queries = list(queries)
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True)
        assert r.returncode == status, r.stderr
        answers = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(answers) == len(queries)
        return answers
    return ask


def test_the_maps_come_from_every_case_table():
    assert {(30, 20), (62, 21), (32, 24), (30, 40), (16, 16), (24, 30), (48, 13), (31, 13)} <= set(MAPS)
    assert len(MAPS) >= 25


def test_an_unknown_query_is_refused(ask):
    assert ask(["dims 30 20", "dims 30", "frobnicate 1", "stage 30 20 4"], status=1) == [cc.dims(30, 20)] + [{"error": "unknown or malformed query"}] * 3


def test_dims_stages_and_padding(ask):
    assert ask("dims %d %d" % m for m in MAPS) == [cc.dims(*m) for m in MAPS]
    for (nf, fs), stages in zip(MAPS, zip(*[iter(ask("stage %d %d %d" % (nf, fs, l) for nf, fs in MAPS for l in range(4)))] * 4)):
        d = cc.dims(nf, fs)
        for l, t in enumerate(stages):
            stride = 2 if l == 2 else 1
            Hi, Wi = d["H%d" % l], d["W%d" % l]
            assert t == dict(Hi=Hi, Wi=Wi, Ho=wc.same_out(Hi, stride), Wo=wc.same_out(Wi, stride), stride=stride, Cin=CHANNELS[l],
                             Cout=CHANNELS[l + 1], pooled=l != 2, relu=l >= 2), (nf, fs, l)
        # the two geometries of tests/wgrad_pmajor_cases.py: conv3 over a2 (stage 2), conv4 over a3 (stage 3)
        for lay, t in zip(wc.layers(nf, fs), stages[2:]):
            assert (lay.H, lay.W, lay.Ho, lay.Wo, lay.stride) == (t["Hi"], t["Wi"], t["Ho"], t["Wo"], t["stride"]), (nf, fs, lay.name)
        # the pooled stages' outputs are the next stage's inputs (a 'valid' 2x2 pool), stage 2's is stage 3's
        assert (stages[0]["Ho"] // 2, stages[1]["Ho"] // 2, stages[2]["Ho"]) == (d["H1"], d["H2"], d["H3"]) and stages[3]["Ho"] // 2 == d["H4"]
    sizes = sorted({v for m in MAPS for k, v in cc.dims(*m).items() if k != "flat" and v > 0})
    cases = [(n, k, s) for n in sizes for k in (1, 3) for s in (1, 2)]
    for (n, k, s), got in zip(cases, ask("pad %d %d %d" % c for c in cases)):
        assert got == dict(out=wc.same_out(n, s), before=wc.same_pad_before(n, k, s)), (n, k, s)
        assert got["before"] == lt.same_pad_before(n, k, s) == lm.pad_before(n, k, s)
    for nf, fs in MAPS:
        c3, c4 = wc.layers(nf, fs)
        got = ask(["pad %d 3 2" % c3.H, "pad %d 3 2" % c3.W, "pad %d 3 1" % c4.H, "pad %d 3 1" % c4.W])
        assert [g["before"] for g in got] == [c3.pt, c3.pl, c4.pt, c4.pl] and (got[0]["out"], got[1]["out"]) == (c3.Ho, c3.Wo)


def _plan_query(row, mode, capturing, training, wants_head, prepared):
    return "plan %d %d %d %d %d %d %d %d %d %d %d %d" % (SIMPLE_CNN, row.nf, row.fs, row.C, HEAD_K, row.B, "fp32" not in mode, "det" in mode,
                                                        capturing, training, wants_head, prepared)


def test_plan_equals_the_restated_flags(ask):
    cases = []
    # beside the rows of the path cases: the maps of tests/wgrad_pmajor_cases.py, one of exactly 16 and one of 20 conv4 pixels among them
    pm_rows = [cc.Row("pm%dx%d" % m, m[0], m[1], 7, 21, False, 0, 0, 1) for m in wc.MAPS]
    for r in pm_rows:
        assert cc.plan_flags(r, "default")["wgrad_pmajor"] == wc.applies(r.nf, r.fs)
    for r in cc.ROWS + pm_rows:
        for row in (r, r._replace(C=48), r._replace(C=49)):
            for mode in PLAN_MODES:
                for capturing in (False, True):
                    cases.append((row, mode, capturing, True, False, False))
                    for wants_head in (False, True):
                        for prepared in (False, True):
                            cases.append((row, mode, capturing, False, wants_head, prepared))
    got = ask(_plan_query(*c) for c in cases)
    for (row, mode, capturing, training, wants_head, prepared), g in zip(cases, got):
        want = cc.plan_flags(row, mode, capturing, training=training, wants_head=wants_head, prepared=prepared)
        assert g == want, (row.name, row.C, mode, capturing, training, wants_head, prepared, {k: (g[k], want[k]) for k in want if g[k] != want[k]})
    # the restatement's "captured" modes are the capturing argument
    assert cc.plan_flags(cc.ROW["b65"], "captured") == cc.plan_flags(cc.ROW["b65"], "default", True) != cc.plan_flags(cc.ROW["b65"], "default")
    # the table is not one-sided: every flag is seen both ways
    for flag in got[0]:
        assert {g[flag] for g in got} == {False, True}, flag


def _dgrad_launches(B, nf, fs):
    """(name, B, H, W, stride, KH, KW) of the three launch_dgrad calls of an exact-fp32 train step (cc.dgrad_mws)"""
    d = cc.dims(nf, fs)
    return (("conv3", B, d["H2"], d["W2"], 2, 3, 3), ("conv4", B, d["H3"], d["W3"], 1, 3, 3), ("dense", B, d["H4"], d["W4"], 1, d["H4"], d["W4"]))


def test_dgrad_classes_and_mw_equal_the_restated_rule(ask):
    simds = 4 * cc.MI355X_CUS
    for r in cc.ROWS:
        launches = _dgrad_launches(r.B, r.nf, r.fs)
        got = ask("dgrad %d %d %d %d %d %d %d" % (l[1:] + (simds,)) for l in launches)
        want_mw = cc.dgrad_mws(r.B, r.nf, r.fs)
        for (name, B, H, W, stride, _, _), g in zip(launches, got):
            rows = cc.parity_class_rows(B, H, W, stride)
            assert g["rc"] == 0 and [B * ny * nx for _, _, ny, nx in g["classes"]] == rows and g["max_rows"] == max(rows), (r.name, name)
            # class (cy, cx) holds the input pixels ih = stride a + cy, iw = stride b + cx: the kernel's decoding (csrc/kws_conv.h)
            assert [tuple(c) for c in g["classes"]] == [(cy, cx, len(range(cy, H, stride)), len(range(cx, W, stride)))
                                                        for cy in range(stride) for cx in range(stride)], (r.name, name)
            assert g["mw"] == want_mw[name] == cc.dgrad_mw(rows, simds), (r.name, name)
    # the first batch of each MW of conv3's launch on either map (tests/test_cnn_paths_host.py), at 1024 SIMDs
    for (nf, fs), want in (((30, 20), {1: 1, 2: 468, 3: 937, 4: 1405}), ((62, 21), {1: 1, 2: 219, 3: 437, 4: 656})):
        d = cc.dims(nf, fs)
        for s in (1024, 256, 1216):
            got = ask("dgrad %d %d %d 2 3 3 %d" % (B, d["H2"], d["W2"], s) for B in range(1, 1406))
            mws = [g["mw"] for g in got]
            assert mws == [cc.dgrad_mw(cc.parity_class_rows(B, d["H2"], d["W2"], 2), s) for B in range(1, 1406)], (nf, fs, s)
            if s == 1024:
                firsts = {}
                for B, mw in zip(range(1, 1406), mws):
                    firsts.setdefault(mw, B)
                assert firsts == want, (nf, fs, firsts)
    # one parity class: the rule of tests/lite_train_cases.py (conv_dgrad<32,16> over stage 2's map, 1 x 1)
    cases = [(c.B, cc.dims(c.nf, c.fs)) for c in lt.CASES]
    got = ask("dgrad %d %d %d 1 1 1 %d" % (B, d["H1"], d["W1"], simds) for B, d in cases)
    assert [g["mw"] for g in got] == [lt.dgrad_mw(B * d["H1"] * d["W1"], cc.MI355X_CUS) for B, d in cases] == [c.mw2 for c in lt.CASES]
    # the two refusals: a stride above 2, more than 8 * stride taps along an axis
    assert ask(["dgrad 4 7 5 3 3 3 1024", "dgrad 4 9 9 1 9 3 1024", "dgrad 4 16 16 2 16 16 1024", "dgrad 4 17 17 2 17 3 1024"]) == \
        [{"rc": 2}, {"rc": 1}, {"rc": 0, "mw": 1, "max_rows": 256, "classes": [[0, 0, 8, 8], [0, 1, 8, 8], [1, 0, 8, 8], [1, 1, 8, 8]]}, {"rc": 1}]


@pytest.mark.parametrize("nf,fs", [m for m in wc.MAPS if wc.applies(*m)])
def test_wgrad_pm_equals_the_restated_plan(ask, nf, fs):
    lay = wc.layers(nf, fs)[1]
    assert (lay.stride, lay.tpb, lay.min_chunks) == (1, 1, 4)
    got = ask("wgrad_pm %d %d %d 1 %d %d" % (B, lay.H, lay.W, wc.MAX_SLOTS, lay.min_chunks) for B in PM_BATCHES)
    for B, g in zip(PM_BATCHES, got):
        want = wc.plan(lay, B)
        assert g == dict(ok=True, pos=want.pos, npos=want.weight, slot0=want.slot0), (nf, fs, B)
    # fewer slots than taps with positions: refused; exactly as many: one slot each
    live = sum(1 for x in wc.plan(lay, 64).weight if x)
    few, enough = ask("wgrad_pm 64 %d %d 1 %d 4" % (lay.H, lay.W, s) for s in (live - 1, live))
    assert few == {"ok": False} and enough["ok"] and enough["slot0"] == wc.plan(lay, 64, max_slots=live).slot0


def test_wgrad_pm_refuses_a_map_of_more_than_16_pixels(ask):
    lay = wc.layers(*wc.FALLBACK)[1]
    assert lay.Ho * lay.Wo == 20
    assert ask("wgrad_pm %d %d %d 1 %d 4" % (B, lay.H, lay.W, wc.MAX_SLOTS) for B in (1, 64, 1400)) == [{"ok": False}] * 3


def test_wgrad_grids_are_one_resident_round_that_covers_every_step(ask):
    cases = [(steps, gy, slots, det) for gy in (1, 3, 9) for slots in SLOTS for det in (0, 1) for steps in SWEEP]
    for (steps, gy, slots, det), g in zip(cases, ask("wgrad %d %d %d %d" % c for c in cases)):
        gx, spw = g["gx"], g["spw"]
        assert gx * 4 * spw >= steps > (gx - 1) * 4 * spw and 1 <= gx <= max(1, slots), (steps, gy, slots, det, g)
        assert gx * gy <= max(gy, slots), (steps, gy, slots, det, g)           # with the tap groups along y: still one round
        if det:
            assert gx == 1
    cases = [(nchunk, ngroups, slots, det) for ngroups in (3, 9) for slots in SLOTS for det in (0, 1) for nchunk in SWEEP]
    for (nchunk, ngroups, slots, det), g in zip(cases, ask("wgrad_bf16 %d %d %d %d" % c for c in cases)):
        assert g["nranges"] % 8 == 0 and g["nranges"] >= 8 and g["nranges"] * g["cpb"] >= nchunk, (nchunk, ngroups, slots, det, g)
        if det:
            assert (g["nranges"], g["cpb"]) == (8, nchunk)


def test_stat_grid_covers_every_row_within_the_partial_slab(ask):
    cases = [(M, C) for C in CHANNELS for M in SWEEP]
    # beyond the sweep: what the steps of tests/lite_train_cases.py hand to stat_grid, its capped cases among them
    cases += sorted({mc for c in lt.CASES for mc in lt.step_stat_grids(c.B, c.nf, c.fs)})
    assert any(lt.stat_capped(M, C) for M, C in cases)
    for (M, C), g in zip(cases, ask("stat %d %d" % c for c in cases)):
        nblk, rows = g["nblk"], g["rows"]
        assert nblk * rows >= M > (nblk - 1) * rows and 1 <= nblk <= lt.STAT_STRIDE, (M, C, g)
        assert (nblk, rows) == lt.stat_grid(M, C), (M, C, g)
        if not lt.stat_capped(M, C):
            assert rows <= 8 * (256 // C)


def test_clip_grids_cover_every_clip(ask):
    cases = [(B, mb) for mb in SLOTS for B in SWEEP]
    for (B, mb), g in zip(cases, ask("even_grid %d %d" % c for c in cases)):
        assert 1 <= g["grid"] <= mb and g["grid"] * -(-B // mb) >= B, (B, mb, g)
    batches = list(SWEEP) + [8192, 8193, 20000, 65536]
    for B, g in zip(batches, ask("l1 %d" % B for B in batches)):
        # at most kStatStride blocks (each leaves one column of the partial slab); a block takes cpb clips, or four waves of cpw clips
        assert 1 <= g["nb"] <= lt.STAT_STRIDE and g["nb"] * g["cpb"] >= B > (g["nb"] - 1) * g["cpb"], (B, g)
        assert 1 <= g["nbm"] <= lt.STAT_STRIDE and g["nbm"] * 4 * g["cpw"] >= B > (g["nbm"] - 1) * 4 * g["cpw"], (B, g)
