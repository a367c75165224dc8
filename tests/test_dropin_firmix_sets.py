"""The filter sets of ear::hip::FirMatrix (libear_amd/host/ear/hip_firmix.hpp: the n_sets constructor, load_set, select, state)
in the C++14 mirror, driven by a C++ program written against the mirror headers alone (tests/cpp/test_dropin_firmix_sets.cpp).
CPU suite: it compiles as C++14 with -Wall -Wextra -Werror.  GPU suite: the one_block shape of tests/firmix_sets_model.py —
a crossfade of one block at the start of a call — leaves the header's formula in the output."""
import os
import re

import pytest

import _dropin


def test_firmix_sets_dropin_program_compiles_as_cpp14(tmp_path):
    assert os.path.exists(_dropin.build(tmp_path, "test_dropin_firmix_sets"))


@pytest.mark.gpu
def test_firmix_sets_dropin_program_passes_on_gpu(tmp_path):
    exe = _dropin.build(tmp_path, "test_dropin_firmix_sets")
    res = _dropin.run(exe, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M), res.stdout
    assert res.stdout.count("worst relative error") == 1, res.stdout
