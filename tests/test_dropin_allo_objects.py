"""ear::hip::AllocentricObjectsGainCalculator (libear_amd/host/ear/hip_allo_objects.hpp) in the C++14 mirror, driven by a C++
program written against the mirror headers alone (tests/cpp/test_dropin_allo_objects.cpp).  CPU suite: it compiles as C++14 with
-Wall -Wextra -Werror, and everything that needs no device passes (ObjectsTypeMetadata with extent, channelLock, divergence and
zones against the rows of the C ABI, each remaining not_implemented by field name, the batch form's refusals, bad values, a
layout without its LFE channels, caller positions).  GPU suite: the whole program, where calculate_device (one device launch)
is held to the host form."""
import re

import pytest

import _dropin


def test_allocentric_objects_calculator_dropin_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_allo_objects")
    res = _dropin.run(exe, "host", timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 60, res.stdout


@pytest.mark.gpu
def test_allocentric_objects_calculator_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_allo_objects")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
