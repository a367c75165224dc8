"""ear::hip::DirectSpeakersGainCalculator and ObjectsProgramme::add_direct_speakers in the C++14 mirror
(libear_amd/host/ear/hip_direct_speakers.hpp, hip_timeline.hpp; earhip group X), driven by a C++ program written against the
mirror headers alone (tests/cpp/test_dropin_direct_speakers_cart.cpp).  CPU suite: it compiles as C++14 and fails loudly
without a GPU.  GPU suite: it runs and every check passes: the Atmos-style bed, locked channels, exceptions by type, and a
programme whose bed is bound by add_direct_speakers rendering bit for bit as one fed the calculator's rows by hand."""

import pytest

import _dropin


def test_direct_speakers_cart_mirror_compiles_as_cxx14_and_fails_loudly_without_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_direct_speakers_cart", wextra=False)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the run is covered by the gpu test")
    res = _dropin.run(exe)
    assert res.returncode != 0
    assert "no" in res.stdout.lower() and "device" in res.stdout.lower()


@pytest.mark.gpu
def test_direct_speakers_cart_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_direct_speakers_cart", wextra=False)
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert " 0 failed" in res.stdout
