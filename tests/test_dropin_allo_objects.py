"""ear::hip::AllocentricObjectsGainCalculator (libear_amd/host/ear/hip_allo_objects.hpp) in the C++14 mirror, driven by a C++
program written against the mirror headers alone (tests/cpp/test_dropin_allo_objects.cpp).  CPU suite: it compiles as C++14 with
-Wall -Wextra -Werror, and everything that needs no device passes (ObjectsTypeMetadata with extent, channelLock, divergence and
zones against the rows of the C ABI, each remaining not_implemented by field name, the batch form's refusals, bad values, a
layout without its LFE channels, caller positions).  GPU suite: the whole program, where calculate_device (one device launch)
is held to the host form."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    from libear_amd import build as build_lib
    build_lib()
    exe = str(tmp_path / "test_dropin_allo_objects")
    libdir = os.path.join(ROOT, "libear_amd", "lib")
    cmd = ["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "libear_amd", "host"),
           os.path.join(ROOT, "tests", "cpp", "test_dropin_allo_objects.cpp"),
           "-L" + libdir, "-learhip", "-Wl,-rpath," + libdir, "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


def test_allocentric_objects_calculator_dropin_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = build(tmp_path)
    res = subprocess.run([exe, "host"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 60, res.stdout


@pytest.mark.gpu
def test_allocentric_objects_calculator_dropin_program_passes_on_gpu(tmp_path):
    exe = build(tmp_path)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
