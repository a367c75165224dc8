"""ear::hip::DelayMatrix (libear_amd/host/ear/hip_delaymix.hpp) in the C++14 mirror, driven by a C++ program written against
the mirror headers alone (tests/cpp/test_dropin_delaymix.cpp).  CPU suite: it compiles as C++14 with -Wall -Wextra -Werror.  GPU
suite: a time alignment of six loudspeakers and an LFE sum fed the rows an ObjectsRenderer returned gives the bits of the
header's operation written out on the host, its host and device forms give the same bits, and configurations outside the
limits are refused.  (The stage is not attached to the renderer: there is no ObjectsRenderer::attach_delaymix to test.)"""
import os
import re

import pytest

import _dropin


def test_delaymix_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_delaymix"))


@pytest.mark.gpu
def test_delaymix_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_delaymix")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("the header's bits") == 1, res.stdout
