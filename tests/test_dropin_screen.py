"""ear::hip::ScreenHandler (libear_amd/host/ear/hip_screen.hpp) in the C++14 mirror, driven by a C++ program written against the
mirror headers alone (tests/cpp/test_dropin_screen.cpp).  CPU suite: it compiles as C++14 with -Wall -Wextra -Werror, and what
needs no device passes (edges and the single-element path with the known answers of include/earhip.h group R, the locks, every
refusal, the pass-through of the default-constructed handler).  GPU suite: the whole program, where the batch path (one device
launch per reference screen) equals the single-element path bit for bit and the gain calculators accept the handler's result."""
import re

import pytest

import _dropin


def test_screen_handler_dropin_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_screen")
    res = _dropin.run(exe, "host", timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 28, res.stdout


@pytest.mark.gpu
def test_screen_handler_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_screen")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
