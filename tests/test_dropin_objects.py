"""ear::hip::ObjectsGainCalculator (libear_amd/host/ear/hip_objects.hpp) in the C++14 mirror, driven by a C++ program written
against the mirror headers alone (tests/cpp/test_dropin_objects.cpp).  CPU suite: it compiles as C++14 with -Wall -Wextra
-Werror.  GPU suite: the known answers of the header for divergence, zone exclusion and channel lock on 4+5+0, the refusals
that remain, and ear::GainCalculatorObjects still refusing all three."""
import os
import re

import pytest

import _dropin


def test_objects_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_objects"))


@pytest.mark.gpu
def test_objects_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_objects")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
