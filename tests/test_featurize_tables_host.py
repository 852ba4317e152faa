"""The featurizer's host tables (csrc/kws_featurize_tables.h) without a device: tests/host/featurize_tables_main.cpp, built here with
the plain C++ compiler, checks the chunk tables, the lane placement, the DCT and the twiddles of every row of tests/geometry_cases.py
and of the default geometry; its bank dumps are held against the reference's bark bank and against the oracle's banks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import featurizer_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "featurize_tables_main.cpp")
BANK_ATOL = 1e-6                    # tests/test_featurizer_gpu.py: test_bark_bank_goldens


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("featurize_tables") / "featurize_tables")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tf-keras-speech-commands_amd", "csrc"), SRC, "-o", exe])
    return exe


def dump_bank(program, kind):
    raw = subprocess.run([program, "--dump-bank", kind], check=True, stdout=subprocess.PIPE).stdout
    return np.frombuffer(raw, np.float32).reshape(20, 513)


def test_rows_of_geometry_cases_are_the_programs_cases():
    """the program restates the table of tests/geometry_cases.py: hold the two together"""
    import re
    import geometry_cases as gc
    text = open(SRC).read()
    for g in gc.ROWS:
        want = '{"%s", %s, %s, %s, %d, %d, %d, %d, KWS_BANK_MEL}' % (g.name, g.buffer_t, "%.3f" % g.window_t, "%.3f" % g.hop_t, g.n_fft, g.n_filt,
                                                                       g.n_mfcc, int(g.use_delta))
        assert re.sub(r"\s+", " ", want) in re.sub(r"\s+", " ", text), want
    assert gc.SAMPLE_RATE == 16000


def test_tables_hold_on_every_geometry(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "11 cases ok" in r.stdout


def test_bark_bank_matches_reference(program, golden):
    np.testing.assert_allclose(dump_bank(program, "bark"), golden["bark_bank_20x513"], rtol=0, atol=BANK_ATOL)


@pytest.mark.parametrize("kind", ["mel", "bark"])
def test_banks_match_oracle(program, kind):
    np.testing.assert_allclose(dump_bank(program, kind), fo.bank(kind), rtol=0, atol=BANK_ATOL)
