"""A hand-built ear::Layout through the gain calculators of the C++14 mirror (libear_amd/host/ear/gain_calculators.hpp,
hip_objects.hpp), driven by a C++ program written against the mirror headers alone (tests/cpp/test_dropin_custom_layout.cpp).
CPU suite: it compiles as C++14 with -Wall -Wextra -Werror, and what needs no device passes (the definitions behind the
calculators, BS.2051 names with their errors).  GPU suite: the whole program — GainCalculatorObjects, ObjectsGainCalculator,
GainCalculatorHOA and GainCalculatorDirectSpeakers on the layout 2+7+0, its withoutLfe() form and a layout without a name."""
import re

import pytest

import _dropin


def test_custom_layout_dropin_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_custom_layout")
    res = _dropin.run(exe, "host", timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 14, res.stdout


@pytest.mark.gpu
def test_custom_layout_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_custom_layout")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
