"""ear::GainCalculatorDirectSpeakers in the C++14 mirror (libear_amd/host/ear/gain_calculators.hpp), driven by a
C++ program written against the mirror headers alone, as a libear application would be
(tests/cpp/test_dropin_direct_speakers.cpp).  CPU suite: it compiles as C++14 and fails loudly without a GPU.
GPU suite: it runs and every check passes."""

import pytest

import _dropin


def test_direct_speakers_mirror_compiles_as_cxx14_and_fails_loudly_without_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_direct_speakers", wextra=False)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the run is covered by the gpu test")
    res = _dropin.run(exe)
    assert res.returncode != 0
    assert "no" in res.stdout.lower() and "device" in res.stdout.lower()


@pytest.mark.gpu
def test_direct_speakers_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_direct_speakers", wextra=False)
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert " 0 failed" in res.stdout
