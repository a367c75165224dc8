"""The extent panner's edge cases without a device (tests/extent_cases.py):
  * the two cores of libear's PolarExtent in the oracle against each other on every group: e_lib, the figure the device's bar is
    made of, stays under its ceiling, so a group cannot loosen its own bar;
  * the float64 model of tests/extent_model.py against the oracle's double core on 4+5+0 (1e-9: both add the same 1652 float64
    terms, the model through numpy's pairwise sums), before it is the reference for the defined layout of group 5;
  * the classification of the chunks (extent_chunk_class of libear_amd/csrc/extent.h), exactly: tests/cpp/extent_host.cpp,
    built by g++ with -Wall -Werror under ASan and UBSan, over group 1's sweeps at steps of 0.05 degrees and groups 2 - 4.

Measured (x86-64, glibc): e_lib is 1.24e-6, 1.06e-6 and 1.14e-6 on group 1 (0+5+0, 9+10+3, 0+2+0), 1.17e-6 and 1.56e-6 on group
2, 7.3e-7 and 6.4e-7 on group 3, 2.9e-7 and 2.2e-7 on group 4; the model on 4+5+0 is within 1.0e-15 of handle(which=1); the host
program finds no violation in 216,030 + 9,284 positions (6.0 million chunks, 1.47 million classed outside, 1.06 million
inside); the smallest slack is 1.000e-3 rad towards r_out + margin and 0.99996e-3 rad towards r_in - margin — the bounds of
extent_setup are tight, and the margin of 1e-3 rad is what is left."""
import os
import subprocess

import numpy as np
import pytest

import _oracle
import custom_layout_model as model
import extent_cases as ec
import extent_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group,layout", [(g, name) for g in (1, 2, 3, 4) for name in ec.layouts_of(g)])
def test_float_core_is_close_to_the_double_core(group, layout):
    ref = ec.reference(group, layout)
    v = ec.columns(ec.cases(group))
    at = ref.worst_at
    print(f"group {group} {layout}: e_lib {ref.e_lib:.3e} over {len(v['az'])} positions, worst at az {v['az'][at]:g} el {v['el'][at]:g} "
          f"dist {v['dist'][at]:g} width {v['width'][at]:g} height {v['height'][at]:g} depth {v['depth'][at]:g}")
    assert 0.0 < ref.e_lib <= (ec.E_LIB_MAX_SWEEP if group == 1 else ec.E_LIB_MAX)
    assert np.isfinite(ref.want).all()
    if layout != "0+2+0":  # (the stereo downmix does not keep the power at the back)
        assert np.abs(np.linalg.norm(ref.want, axis=1) - 1.0).max() <= 1e-9


def test_cases_say_what_they_claim():
    """the thresholds the table places cases on are where extent.h has them"""
    sweeps = ec.cases(1)
    assert len(sweeps) == len(ec.DIRECTIONS) * len(ec.HEIGHT_RULES) and all(len(c.width) == 1441 for c in sweeps)
    assert all(c.width[0] == 0.0 and c.width[-1] == 360.0 and (c.dist == 1.0).all() and not c.depth.any() for c in sweeps)
    by_name = {c.name: c for c in ec.cases(2)}
    circ = by_name["circular"]
    half = np.radians(circ.width[circ.dist == 1.0] - circ.height[circ.dist == 1.0]) / 2.0  # (distance 1 leaves an extent as it is)
    assert (np.abs(half) < 1e-6).any() and (half >= 1e-6).any() and (half <= -1e-6).any()
    assert _oracle.extent_mod(40.0, 1.0) == 40.0 and _oracle.extent_mod(0.0, 0.5) > 0.0 and _oracle.extent_mod(0.0, 1.0) == 0.0
    # the near pass of group 3 reaches distance 0 (clamped) and the origin is there
    v = ec.columns(ec.cases(3))
    assert ((v["dist"] - v["depth"] / 2.0) < 0.0).any() and (v["dist"] == 0.0).any() and (v["dist"] == 1e-12).any()
    # either side of the pole rule
    el = ec.cases(4)[0].el
    assert (90.0 - np.abs(el) < 1e-5).any() and ((90.0 - np.abs(el) > 1e-5) & (90.0 - np.abs(el) < 1e-3)).any()
    # group 6: every other position has nothing to spread
    for n in ec.CALL_SIZES:
        c = ec.small_call(n)
        quiet = (c.width == 0.0) & (c.height == 0.0) & (c.dist == 1.0) & (c.depth == 0.0)
        assert quiet[1::2].all() and not quiet[0::2].any() and len(c.az) == n
    assert ec.BATCH == 1 << 18


def test_wide_layouts():
    """group 5's layout is the widest a definition may be, with LFE channels inside the list; 30 loudspeakers are refused"""
    from libear_amd import capi
    assert len(ec.WIDE) == 32 and sum(1 for c in ec.WIDE if not c[3]) == 22
    real = [i for i, c in enumerate(ec.WIDE) if not c[3]]
    assert real != list(range(22)) and real[-1] == 31
    capi.define_layout("wide 22", ec.WIDE)
    assert len(capi.layout_channels("wide 22")) == 32
    assert len(ec.TOO_WIDE) == 32 and sum(1 for c in ec.TOO_WIDE if not c[3]) == 30
    with pytest.raises(capi.EarHipError) as info:
        capi.define_layout("wide 30", ec.TOO_WIDE)
    assert info.value.code == capi.NOT_IMPLEMENTED and "more than 22 loudspeakers" in str(info.value)
    assert len(ec.wide_positions().az) == 64


def test_model_equals_the_double_core():
    """tests/extent_model.py over custom_layout_model's panner of 4+5+0 against handle(which=1), at group 5's positions"""
    from libear_amd import capi
    channels = capi.layout_channels("4+5+0")
    c = ec.wide_positions()
    xyz = _oracle.cart(c.az, c.el, c.dist)
    got = extent_model.PolarExtent(lambda p: model.Panner(channels).pan(p)[0]).handle(xyz, c.width, c.height, c.depth)
    want = _oracle.PolarExtent("4+5+0").handle(xyz, c.width, c.height, c.depth, which=1)
    worst = float(ec.rel(got, want).max())
    print(f"model against handle(which=1) on 4+5+0: {worst:.3e}")
    assert got.shape == want.shape == (64, 9) and worst <= 1e-9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("extent_host") / "extent_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "extent_host.cpp"), "-o", str(path)], check=True)
    return str(path)


def run_host(exe, tmp_path, rows):
    src = tmp_path / "rows.bin"
    src.write_bytes(np.ascontiguousarray(rows, np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    words = res.stdout.split()
    return res.returncode, dict(zip(words[0::2], (float(w) for w in words[1::2]))), res.stderr


HOST_SETS = {"sweeps at 0.05": lambda: np.concatenate([rows for _, _, rows in ec.sweep_rows(0.05)]),
             "groups 2 - 4": lambda: np.stack(list(ec.columns(ec.cases(2) + ec.cases(3) + ec.cases(4)).values()), axis=1)}


@pytest.mark.parametrize("which", sorted(HOST_SETS))
def test_chunk_classes_are_exact(exe, tmp_path, which):
    """a chunk classed outside weighs 0.0f at each of its points, one classed inside 1.0f; the slack left is positive"""
    rows = HOST_SETS[which]()
    code, got, err = run_host(exe, tmp_path, rows)
    print(which, got)
    assert code == 0 and got["violations"] == 0, err
    assert got["positions"] == len(rows) and got["renderings"] >= 0.9 * len(rows)
    # the shortcut is taken, both ways, and not always
    assert got["outside"] > 0 and got["inside"] > 0 and got["edge"] > 0
    assert got["slack_out"] > 0.0 and got["slack_in"] > 0.0
