"""The C++14 mirror of libear's ear::dsp interfaces (libear_amd/host/ear/...), driven by a C++
program that restates the reference's own Catch2 tests (tests/cpp/test_dropin.cpp).
CPU suite: the headers compile as C++14 and link against libearhip.so, and the program fails
loudly without a GPU.  GPU suite: the program runs and every check passes."""

import pytest

import _dropin


def test_mirror_headers_compile_as_cxx14_and_fail_loudly_without_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin", wextra=False, libs=("dl",))
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the run is covered by the gpu test")
    res = _dropin.run(exe)
    assert res.returncode != 0
    assert "no" in res.stdout.lower() and "device" in res.stdout.lower()


@pytest.mark.gpu
def test_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin", wextra=False, libs=("dl",))
    res = _dropin.run(exe, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert " 0 failed" in res.stdout
