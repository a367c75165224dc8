"""ear/hip_timeline.hpp (BlockTiming, timelinePoints, timelineWindow, ObjectsProgramme) and ObjectsRenderer::set_object[s]_blocks
in the C++14 mirror, driven by a C++ program written against the mirror headers alone (tests/cpp/test_timeline.cpp).  CPU suite:
it compiles as C++14 with -Wall -Wextra -Werror, and what needs no device passes (timelinePoints and timelineWindow on cases
worked out by hand, the refusals).  GPU suite: the whole program, where ObjectsProgramme::bind of a polar track, a Cartesian track
and a stepped bed — whole, by window, behind a reproduction screen — renders bit for bit as the calculators, the screen stage,
timelinePoints and set_object_points called by hand."""
import re

import pytest

import _dropin


def test_timeline_mirror_program_compiles_as_cpp14_and_its_host_part_passes(tmp_path):
    exe = _dropin.build(tmp_path, "test_timeline")
    res = _dropin.run(exe, "host", timeout=120)
    m = re.search(r"^host: (\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert res.returncode == 0 and m and int(m.group(1)) >= 20, res.stdout


@pytest.mark.gpu
def test_timeline_mirror_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_timeline")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"^(\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 34, res.stdout
