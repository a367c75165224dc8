"""ear::conversion in the C++14 mirror (libear_amd/host/ear/conversion.hpp), driven by a C++ program written against
the mirror headers alone, as a libear application would be (tests/cpp/test_dropin_conversion.cpp).  CPU suite: it
compiles as C++14 with -Wall -Werror, every single-element check passes, and the batch overloads fail loudly without a
GPU.  GPU suite: the whole program passes."""
import re

import pytest

import _dropin


def test_conversion_mirror_single_element_passes_without_gpu_and_batch_fails_loudly(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_conversion", wextra=False)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the run is covered by the gpu test")
    res = _dropin.run(exe, timeout=120)
    m = re.search(r"single-element: (\d+) passed, 0 failed", res.stdout)
    assert m and int(m.group(1)) >= 50, res.stdout
    assert res.returncode != 0
    assert "FAILED: batch" in res.stdout and "no" in res.stdout.lower() and "device" in res.stdout.lower()


@pytest.mark.gpu
def test_conversion_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_conversion", wextra=False)
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
