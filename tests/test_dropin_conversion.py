"""ear::conversion in the C++14 mirror (libear_amd/host/ear/conversion.hpp), driven by a C++ program written against
the mirror headers alone, as a libear application would be (tests/cpp/test_dropin_conversion.cpp).  CPU suite: it
compiles as C++14 with -Wall -Werror, every single-element check passes, and the batch overloads fail loudly without a
GPU.  GPU suite: the whole program passes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    from libear_amd import build as build_lib
    build_lib()
    exe = str(tmp_path / "test_dropin_conversion")
    libdir = os.path.join(ROOT, "libear_amd", "lib")
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "libear_amd", "host"),
           os.path.join(ROOT, "tests", "cpp", "test_dropin_conversion.cpp"),
           "-L" + libdir, "-learhip", "-Wl,-rpath," + libdir, "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


def test_conversion_mirror_single_element_passes_without_gpu_and_batch_fails_loudly(tmp_path):
    exe = build(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the run is covered by the gpu test")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    m = re.search(r"single-element: (\d+) passed, 0 failed", res.stdout)
    assert m and int(m.group(1)) >= 50, res.stdout
    assert res.returncode != 0
    assert "FAILED: batch" in res.stdout and "no" in res.stdout.lower() and "device" in res.stdout.lower()


@pytest.mark.gpu
def test_conversion_dropin_program_passes_on_gpu(tmp_path):
    exe = build(tmp_path)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
