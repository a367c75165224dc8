"""CPU checks of the biquad filter matrix (include/earhip.h, group O): the designer against scipy, the two host forms of the
shared maths header (libear_amd/csrc/iir.h: what the device kernels run — sample by sample, and chunked in the kernels' order
of operations) compiled for the host under ASan and UBSan against the float64 model (tests/iir_model.py) under the header's
bound, for every cutting of the stream; every refusal of earhip_iir_create without a device; the new symbols declared, exported
and bound.

The bound: |y - ref64| <= 2^-24 |ref64| + 1e-9 * (peak of that output row).  Measured by these tests over all 30 output rows
(four signals x seven filters, a summed row, an empty row) at 48 kHz, 33,613 samples, the same for every cutting (one call,
around the chunk length, short calls back to back, two halves off the grid):
                         worst error / bound     the error beyond the float32 rounding, as a share of the row's peak
    sequential form      0.982                   1.6e-12
    chunked form         0.982                   1.3e-11 (8.9e-12 for the two halves)
The first column is the rounding to float32 (half an ulp is up to 2^-24 |ref| just above a power of two, so it approaches 1
for any correct implementation); the second is what the 1e-9 term is for, and the chunked form sits 75x inside it.  sosfilt
lies 6.8e-13 of the peak from a long-double run of the recurrence on the LR4 low-pass at 20 Hz (asserted: 30x inside 1e-9)."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import butter, sosfreqz

import iir_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48000.0
LC = 256  # (asserted against the header's constant below)
N = 131 * LC + 77  # two scan groups of 64 chunks and a bit


def signals(n=N):
    x = np.zeros((4, n), np.float32)
    x[0] = (0.25 * np.random.default_rng(11).standard_normal(n)).astype(np.float32)
    x[1, 100:] = 0.5  # a step
    x[2, 37] = 1.0    # an impulse
    return x          # (row 3: silence)


def six_sections():
    from libear_amd import capi
    return np.concatenate([im.lr4("lowpass", 80.0, FS), [capi.iir_design("peaking", FS, 200.0, 2.0, 6.0)],
                           [capi.iir_design("peaking", FS, 1000.0, 1.0, -4.0)], im.butter_sections(4, 30.0, FS, "highpass")])


def filters():
    return {"LR4 high 20": im.lr4("highpass", 20.0, FS), "LR4 low 20": im.lr4("lowpass", 20.0, FS),
            "LR4 high 80": im.lr4("highpass", 80.0, FS), "LR4 low 80": im.lr4("lowpass", 80.0, FS),
            "Butterworth 8 low 40": im.butter_sections(8, 40.0, FS), "six sections": six_sections(), "gain only": None}


def bank():
    """(n_out, routes, row names): every signal through every filter into a row of its own, then a row that sums five routes,
    then a row without a route"""
    routes, names = [], []
    for fname, sec in filters().items():
        for s, sname in enumerate(("gaussian", "step", "impulse", "silence")):
            routes.append((s, len(names), -0.7 if fname == "gain only" else 1.0, sec))
            names.append(f"{fname} / {sname}")
    k = len(names)
    routes += [(0, k, 0.5, im.lr4("lowpass", 80.0, FS)), (1, k, -1.25, None), (2, k, 2.0, im.lr4("highpass", 80.0, FS)),
               (0, k, 1.0, None), (0, k, 0.3, six_sections())]
    names += ["summed", "no route"]
    return len(names), routes, names


_cache = {}


def reference():
    if "ref" not in _cache:
        n_out, routes, names = bank()
        x = signals()
        _cache["ref"] = (x, n_out, routes, names, im.model(x, n_out, routes))
    return _cache["ref"]


def test_designer_lowpass_and_highpass_are_scipys_butterworth():
    from libear_amd import capi
    for fs in (44100.0, 48000.0, 96000.0):
        for f0 in (20.0, 80.0, 120.0, 1000.0):
            for kind in ("lowpass", "highpass"):
                want = im.sections_of(butter(2, f0, btype=kind, fs=fs, output="sos"))[0]
                got = capi.iir_design(kind, fs, f0, im.Q_BUTTER)
                assert np.abs(got - want).max() <= 1e-12, (fs, f0, kind, got, want)


def _mag_db(section, fs, freqs):
    w = 2 * np.pi * np.asarray(freqs, np.float64) / fs
    return 20 * np.log10(np.abs(sosfreqz(im.sos_of(section), worN=w)[1]))


def test_designer_peaking_and_shelves_by_their_magnitudes():
    from libear_amd import capi
    fs = 48000.0
    for f0, q, g in ((100.0, 0.7, 6.0), (1000.0, 2.0, -9.0), (8000.0, 1.0, 3.0)):
        at = _mag_db(capi.iir_design("peaking", fs, f0, q, g), fs, [0.0, f0, fs / 2])
        assert np.allclose(at, [0.0, g, 0.0], rtol=0, atol=1e-9), ("peaking", f0, at)
        at = _mag_db(capi.iir_design("low_shelf", fs, f0, im.Q_BUTTER, g), fs, [0.0, f0, fs / 2])
        assert np.allclose(at, [g, g / 2, 0.0], rtol=0, atol=1e-9), ("low shelf", f0, at)
        at = _mag_db(capi.iir_design("high_shelf", fs, f0, im.Q_BUTTER, g), fs, [0.0, f0, fs / 2])
        assert np.allclose(at, [0.0, g / 2, g], rtol=0, atol=1e-9), ("high shelf", f0, at)


def test_designer_lr4_low_plus_high_is_an_allpass():
    from libear_amd import capi
    for fs, f0 in ((48000.0, 80.0), (44100.0, 120.0), (96000.0, 1000.0)):
        w = np.linspace(0.0, np.pi, 4001)
        lo = np.concatenate([[capi.iir_design("lowpass", fs, f0, im.Q_BUTTER)]] * 2)
        hi = np.concatenate([[capi.iir_design("highpass", fs, f0, im.Q_BUTTER)]] * 2)
        h = sosfreqz(im.sos_of(lo), worN=w)[1] + sosfreqz(im.sos_of(hi), worN=w)[1]
        assert np.abs(np.abs(h) - 1.0).max() <= 1e-9, (fs, f0)


def test_designer_refusals():
    from libear_amd import capi
    nan, inf = float("nan"), float("inf")
    for args in (("lowpass", 48000.0, 0.0), ("lowpass", 48000.0, 24000.0), ("lowpass", 48000.0, -5.0), ("lowpass", 48000.0, 100.0, 0.0),
                 ("lowpass", 48000.0, 100.0, -1.0), ("lowpass", nan, 100.0), ("lowpass", 48000.0, nan), ("peaking", 48000.0, 100.0, 1.0, inf),
                 ("lowpass", 48000.0, 100.0, nan), ("lowpass", 0.0, 100.0), (5, 48000.0, 100.0), (-1, 48000.0, 100.0), ("notch", 48000.0, 100.0)):
        with pytest.raises(capi.InvalidArgument):
            capi.iir_design(*args)
    assert capi.load().earhip_iir_design(0, 48000.0, 100.0, 1.0, 0.0, None) == capi.INVALID_ARGUMENT


def test_the_model_against_a_long_double_run():
    x = signals(12000)[0]
    sec = im.lr4("lowpass", 20.0, FS)
    ref = im.model(x[None, :], 1, [(0, 0, 1.0, sec)])[0]
    ld = im.long_double_run(x, sec).astype(np.float64)
    spread = np.abs(ref - ld).max() / np.abs(ref).max()
    print(f"sosfilt against the long-double recurrence, LR4 low 20 Hz: {spread:.2e} of the peak")
    assert spread <= 1e-9 / 30


@pytest.mark.parametrize("chunked", [False, True], ids=["sequential", "chunked"])
def test_host_forms_against_the_model_under_every_cutting(chunked):
    x, n_out, routes, names, ref = reference()
    assert im.host_exe() and LC == int(re.search(r"kIirChunk = (\d+);", open(os.path.join(ROOT, "libear_amd", "csrc", "iir.h")).read()).group(1))
    for cut, calls in im.cuttings(x.shape[1], LC).items():
        y = im.host_run(x, n_out, routes, calls, chunked)
        again = im.host_run(x, n_out, routes, calls, chunked)
        assert np.array_equal(y.view(np.uint32), again.view(np.uint32)), cut  # the same cutting twice: the same bits
        worst = max(im.worst_ratio(y[k], ref[k]) for k in range(n_out))
        peaks = np.abs(ref).max(axis=1)
        live = peaks > 0
        f64 = (np.abs(y.astype(np.float64) - ref) - 2.0 ** -24 * np.abs(ref)).max(axis=1)[live] / peaks[live]
        print(f"{'chunked' if chunked else 'sequential'}, {cut}: worst error {worst:.3f} of the bound; beyond the rounding "
              f"{max(f64.max(), 0.0):.1e} of the peak")
        for k in range(n_out):
            r = im.worst_ratio(y[k], ref[k])
            assert r <= 1.0, (cut, names[k], r)
        assert np.all(y[-1].view(np.uint32) == 0), cut                      # no route: exactly +0.0
        assert np.all(y[[3, 7, 11, 15, 19, 23, 27]] == 0), cut             # silence in, silence out


def test_host_program_refuses_what_create_refuses():
    x = np.zeros((2, 8), np.float32)
    ok = im.lr4("lowpass", 80.0, FS)
    for routes, word in (([(0, 0, 1.0, [[1, 0, 0, 0.0, 1.0]])], "stable"), ([(0, 0, 1.0, [[1, 0, 0, 2.0, 0.99]])], "stable"),
                         ([(0, 0, 1.0, [[1, 0, 0, -1.5, 0.5]])], "stable"), ([(0, 0, float("nan"), ok)], "finite"),
                         ([(0, 0, 1.0, [[float("inf"), 0, 0, 0, 0]])], "finite"), ([(2, 0, 1.0, ok)], "in must"),
                         ([(0, 1, 1.0, ok)], "out must"), ([(-1, 0, 1.0, ok)], "in must"), ([], "n_routes")):
        assert word in im.host_run(x, 1, routes, expect=3), (routes, word)


NEW_SYMBOLS = ["earhip_iir_create", "earhip_iir_destroy", "earhip_iir_reset", "earhip_iir_info", "earhip_iir_process_device",
               "earhip_iir_process", "earhip_iir_design"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
    assert "typedef struct earhip_iir_config" in header and "typedef struct earhip_iir_route" in header
    from libear_amd import capi
    assert hasattr(capi, "IirBank") and hasattr(capi, "iir_design")


def test_bindings_refuse_bad_arguments_without_a_device():
    """the configuration is checked before the context is looked at: every refusal of earhip_iir_create on any machine"""
    from libear_amd import capi
    ok = im.lr4("lowpass", 80.0, FS)
    nan, inf = float("nan"), float("inf")
    good = dict(n_in=2, n_out=3, routes=[(0, 0, 1.0, ok), (1, 2, 0.5, None)], max_samples=1000)
    nine = np.concatenate([ok] * 5)[:9]
    bad = [dict(n_in=0), dict(n_in=65), dict(n_out=0), dict(n_out=65), dict(routes=[]), dict(routes=[(0, 0, 1.0, None)] * 513),
           dict(max_samples=0), dict(max_samples=-1), dict(n_in=True), dict(n_out=2.5),
           dict(routes=[(2, 0, 1.0, ok)]), dict(routes=[(-1, 0, 1.0, ok)]), dict(routes=[(0, 3, 1.0, ok)]), dict(routes=[(0, -1, 1.0, ok)]),
           dict(routes=[(0, 0, nan, ok)]), dict(routes=[(0, 0, inf, None)]), dict(routes=[(0, 0, 1.0, nine)]),
           dict(routes=[(0, 0, 1.0, [[1, 0, 0, 0.0, 1.0]])]), dict(routes=[(0, 0, 1.0, [[1, 0, 0, 0.0, -1.0]])]),
           dict(routes=[(0, 0, 1.0, [[1, 0, 0, 1.5, 0.5]])]), dict(routes=[(0, 0, 1.0, [[1, 0, 0, -1.5, 0.5]])]),
           dict(routes=[(0, 0, 1.0, [[nan, 0, 0, 0, 0]])]), dict(routes=[(0, 0, 1.0, [[1, 0, inf, 0, 0]])]),
           dict(routes=[(0, 0, 1.0, [[1, 0, 0, nan, 0]])]), dict(routes=[(0, 0, 1.0, [[1, 0, 0]])]), dict(routes=[(0, 0, 1.0)]),
           dict(routes=[(0, 0, 1.0, ok), (0, 0, 1.0, [[1, 0, 0, 0, 1.0]])])]
    for kw in bad:
        with pytest.raises(capi.InvalidArgument):
            capi.IirBank(None, **dict(good, **kw))
    with pytest.raises(capi.InvalidArgument, match="ctx"):
        capi.IirBank(None, **good)  # (a good configuration gets as far as the missing context)
    lib = capi.load()
    assert lib.earhip_iir_reset(None) == capi.INVALID_ARGUMENT and lib.earhip_iir_destroy(None) == capi.OK
    assert lib.earhip_iir_info(None, None) == capi.INVALID_ARGUMENT and lib.earhip_iir_create(None, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_iir_process(None, 0, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_iir_process_device(None, 0, None, 0, None, 0) == capi.INVALID_ARGUMENT
