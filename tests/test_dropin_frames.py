"""ObjectsRenderer::process_frames in the C++14 mirror (libear_amd/host/ear/dsp/objects_renderer.hpp), driven by a C++ program
written against the mirror headers alone (tests/cpp/test_dropin_frames.cpp).  CPU suite: it compiles as C++14 with -Wall -Werror.
GPU suite: s16 and s24 frames render bit-identically to process() on the converted rows."""
import os
import re

import pytest

import _dropin


def test_frames_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_frames", wextra=False))


@pytest.mark.gpu
def test_frames_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_frames", wextra=False)
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("bit-identical") == 4, res.stdout
