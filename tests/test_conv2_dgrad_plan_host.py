"""Where plan_cnn (csrc/kws_cnn_plan.h) picks the compile-time kernels of conv2's backward, without a device: tests/host/cnn_plan_dgrad_main.cpp,
built here with the plain C++ compiler, prints dgrad2_fast (kws_conv2_dgrad_fast.h) and wgrad2_fast (kws_conv2_wgrad_fast.h) of the training
plan for every row of tests/cnn_path_cases.py in the modes default / det / fp32 / capturing.  The two kernels are built for the same map
and take their BatchNorm coefficients from the same accumulator set, so the flags agree everywhere, and both are set only for the default
30 x 20 feature map (a 15 x 10 conv2 map) in default mode: deterministic mode, a captured step, the fp32 mode and every other map keep the
runtime-geometry kernels."""
import json
import os
import shutil
import subprocess

import pytest

import cnn_path_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "cnn_plan_dgrad_main.cpp")
SIMPLE_CNN, HEAD_K = 0, 128                         # KWS_SIMPLE_CNN; the Dense layer in front of simple_cnn's head
# mode -> (mprec, det, capturing)
MODES = {"default": (1, 0, 0), "det": (1, 1, 0), "fp32": (0, 0, 0), "capturing": (1, 0, 1)}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("cnn_plan_dgrad") / "cnn_plan_dgrad")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tf-keras-speech-commands_amd", "csrc"), SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and not r.stdout.strip(), "the host program must build without a warning:\n" + r.stdout
    cases = [(row, mode) for row in cc.ROWS for mode in MODES]
    queries = ["%d %d %d %d %d %d %d %d %d" % ((SIMPLE_CNN, row.nf, row.fs, row.C, HEAD_K, row.B) + MODES[mode]) for row, mode in cases]
    r = subprocess.run([exe], input="".join(q + "\n" for q in queries + ["1 2 3"]), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 1, r.stderr                # the malformed last line, and nothing else
    got = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(got) == len(cases) + 1 and "error" in got[-1] and not any("error" in g for g in got[:-1])
    return list(zip(cases, got[:-1]))


def test_the_two_flags_agree_everywhere(answers):
    for (row, mode), g in answers:
        assert g["dgrad2_fast"] == g["wgrad2_fast"], (row.name, mode, g)


def test_both_are_set_only_for_the_default_map_in_default_mode(answers):
    seen = set()
    for (row, mode), g in answers:
        assert (g["H1"], g["W1"]) == (row.nf // 2, row.fs // 2), (row.name, g)
        default_map = (g["H1"], g["W1"]) == (15, 10)     # conv2's map of the 30 x 20 features (and of 31 or 21: the pool drops the odd row / column)
        want = default_map and mode == "default"
        assert g["dgrad2_fast"] == want and g["wgrad2_fast"] == want, (row.name, row.nf, row.fs, row.B, mode, g)
        seen.add((default_map, mode, want))
    # the table is not one-sided: the default map in every mode, another map in default mode
    assert {(True, m, m == "default") for m in MODES} <= seen and (False, "default", False) in seen
