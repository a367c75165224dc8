"""ear::hip::SampleRateConverter (libear_amd/host/ear/hip_src.hpp) in the C++14 mirror, driven by a C++ program written against
the mirror headers alone (tests/cpp/test_dropin_src.cpp).  CPU suite: it compiles as C++14 with -Wall -Wextra -Werror.  GPU
suite: a converter from 48 kHz to 44.1 kHz fed the rows an ObjectsRenderer returned gives the bits of the header's operation
written out on the host and ceil(N L / M) outputs, its host and device forms give the same bits, and configurations outside the
limits are refused.  (The stage is not attached to the renderer: there is no ObjectsRenderer::attach_src to test.)"""
import os
import re

import pytest

import _dropin


def test_src_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_src"))


@pytest.mark.gpu
def test_src_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_src")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("the header's bits") == 1, res.stdout
