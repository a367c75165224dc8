"""ear::hip::ScreenHandler::apply_cartesian (libear_amd/host/ear/hip_screen.hpp) in the C++14 mirror, driven by a C++ program
written against the mirror headers alone (tests/cpp/test_dropin_screen_cart.cpp).  CPU suite: it compiles as C++14 with -Wall
-Wextra -Werror, and what needs no device passes (the single-block form against the bits of the C entry point of include/earhip.h
group V, screenRef cleared and every other field untouched, the locks, each refusal by field name, ScreenHandler::apply still
refusing Cartesian blocks, the pass-through of the default-constructed handler).  GPU suite: the whole program, where the batch
form (one device launch per reference screen) is held to the single form within 1e-6 per coordinate and
AllocentricObjectsGainCalculator accepts its result."""
import re

import pytest

import _dropin


def test_cartesian_screen_handler_dropin_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_screen_cart")
    res = _dropin.run(exe, "host", timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 24, res.stdout


@pytest.mark.gpu
def test_cartesian_screen_handler_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_screen_cart")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"^(\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 40, res.stdout
