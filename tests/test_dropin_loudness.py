"""ear::hip::LoudnessMeter (libear_amd/host/ear/hip_loudness.hpp) and ObjectsRenderer::attach_loudness in the C++14 mirror,
driven by a C++ program written against the mirror headers alone (tests/cpp/test_dropin_loudness.cpp).  CPU suite: it compiles
as C++14 with -Wall -Wextra -Werror.  GPU suite: the attached meter holds the step energies of the header's cascade."""
import os
import re

import pytest

import _dropin


def test_loudness_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_loudness"))


@pytest.mark.gpu
def test_loudness_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_loudness")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("worst relative difference") == 2, res.stdout
