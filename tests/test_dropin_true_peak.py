"""True peak and loudness range through ear::hip::LoudnessMeter (libear_amd/host/ear/hip_loudness.hpp) in the C++14 mirror,
driven by a C++ program written against the mirror headers alone (tests/cpp/test_dropin_true_peak.cpp).  CPU suite: it compiles
as C++14 with -Wall -Wextra -Werror.  GPU suite: a meter attached to a renderer holds the peaks of the header's interpolator."""
import os
import re

import pytest

import _dropin


def test_true_peak_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_true_peak"))


@pytest.mark.gpu
def test_true_peak_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_true_peak")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("of the bound") == 2, res.stdout
