"""The host pipeline of long calls from host memory (libear_amd/csrc/host_pipeline.h: the staging threads and the chunk loop) on
the CPU: tests/cpp/test_host_pipeline.cpp drives the real pool and the real loop against lanes made of threads and memcpy — row and
range jobs, 1 / 3 / 8 staging threads, 1 ... kMaxChunks chunks, back-to-back calls, two pipelines at once, pool lifetimes, a
failure injected at every stage, the order of a call's stages — built once with the thread sanitizer and once with the address and
undefined-behaviour sanitizers.  A stand-alone program: nothing here is loaded into Python, and the environment is passed on as it
is."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "libear_amd", "csrc")]
SANITIZERS = {
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"],
}


@pytest.mark.parametrize("name", list(SANITIZERS))
def test_host_pipeline_on_cpu(tmp_path, name):
    exe = tmp_path / f"test_host_pipeline_{name}"
    src = os.path.join(ROOT, "tests", "cpp", "test_host_pipeline.cpp")
    subprocess.run(["g++", *FLAGS, *SANITIZERS[name], src, "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"(\d+) cases, 0 failed", res.stdout)
    assert m and int(m.group(1)) > 500, res.stdout
    assert "Sanitizer" not in res.stdout, res.stdout
