"""The case table of the decorrelator stage (K2) off its default operating point: block size, compensation delay, FIR length,
cuttings of the stream into calls, context options and the plan of the stage each case must run (the kernel form among them),
shared by tests/test_render_delay_cpu.py (the two references against each other) and tests/test_gpu_render_delay.py.

Plain Python: nothing here needs a device.  The expected plans are WRITTEN DOWN from libear_amd/csrc/decor_plan.h and
decor_stage.h, not computed by the library:

  Bk    partition size of the FIRs: the block size B, or 512 for B = 1024, 2048, 4096 with at most 512 taps (unless K2_OWN_BLOCK)
  NP    ceil(n_taps / Bk) partitions
  form  WAVE for Bk = 512 and NP = 1 (unless K2_WG), else WG for 2 Bk a power of two from 128, else RT (run-time shape)
  run   blocks per run: option RUN (made odd) where given; else the wave kernel's own choice, which is 1 for every call here (a
        call of these sizes is less than one round of workgroups on any chip of ten compute units and more, where one pair of blocks
        per run is the cheapest: wave_run_len), 7 for the workgroup kernel at 2 Bk = 2048, 11 at every other size.

Within the workgroup template (form WG) the transform size picks the variant: 2 Bk = 1024 `kTwInRegs`, 2048 `kFused2k`, every
other size the generic one (at 2 Bk <= 2048 with the twiddles in LDS; Bk = 64: fewer samples than threads).
"""
from collections import namedtuple

WG, RT, WAVE = 0, 1, 2

Case = namedtuple("Case", "id group B D n_taps nblocks cuttings opts layout plan")

# blocks per case (at most 24 blocks and 8192 samples), and the ragged cutting: it begins [1, 1, 2] so that a delay of
# 3 B + 5 is longer than each of the first calls and than the first two together, and has one call of more than 11 blocks
# where the total allows it (two runs of the workgroup kernel in one call: a run whose `first` is > 0)
NBLOCKS = {16: 24, 32: 24, 64: 24, 256: 16, 480: 16, 512: 16, 1024: 8, 2048: 4}
RAGGED = {24: [1, 1, 2, 13, 7], 16: [1, 1, 2, 12], 8: [1, 1, 2, 3, 1], 4: [1, 1, 2]}


def cuttings(nblocks):
    """the whole stream in one call, every block its own call, one ragged list"""
    return ([nblocks], [1] * nblocks, RAGGED[nblocks])


def delays(B, extra=()):
    """0 (two buses), 1, around the block size, longer than two blocks, longer than the first calls of the ragged cutting; from
    block 128 B - 1, B + 1 and 2 B + 3 are no multiples of 4, and a multiple of 64 is among them (B itself, or `extra`)"""
    return [0, 1, B - 1, B, B + 1, 2 * B + 3, 3 * B + 5] + list(extra)


# (group, B, n_taps, options, plan (Bk, NP, form, run), delays): one row per way of reaching a kernel form; a case per delay
FORMS = [
    # wave kernel: 512-sample partitions, one partition.  63 / 65: a lane row of the first block from the state, short of one
    # sample and one sample more; 256 / 257: the two ways it publishes the delay line
    ("wave-512", 512, 512, {}, (512, 1, WAVE, 1), delays(512, (63, 65, 256, 257))),
    # ... for blocks of 1024 and 2048 whose FIRs fit a partition: the delays around Bk = 512 as well as around B
    ("wave-1024", 1024, 512, {}, (512, 1, WAVE, 1), delays(1024, (511, 513))),
    ("wave-2048", 2048, 512, {}, (512, 1, WAVE, 1), [0, 513, 2047, 2049, 3 * 2048 + 5]),
    # workgroup kernel, L = 1024 (kTwInRegs)
    ("wg1024-k2wg", 512, 512, {"EARHIP_K2_WG": "1"}, (512, 1, WG, 11), delays(512)),
    ("wg1024-513taps", 512, 513, {}, (512, 2, WG, 11), [0, 511, 513, 3 * 512 + 5]),
    # workgroup kernel, L = 2048 (kFused2k)
    ("wg2048-own", 1024, 512, {"EARHIP_K2_OWN_BLOCK": "1"}, (1024, 1, WG, 7), delays(1024)),
    ("wg2048-513taps", 1024, 513, {}, (1024, 1, WG, 7), [0, 1023, 1025, 3 * 1024 + 5]),
    # workgroup kernel, generic variant, fewer samples than threads (two partitions: the history state)
    ("wg128", 64, 100, {}, (64, 2, WG, 11), delays(64)),
    # workgroup kernel, generic variant
    ("wg512", 256, 512, {}, (256, 2, WG, 11), delays(256)),
    # ... twiddles not in LDS (L = 4096)
    ("wg4096-own", 2048, 512, {"EARHIP_K2_OWN_BLOCK": "1"}, (2048, 1, WG, 11), [0, 2047, 2049, 3 * 2048 + 5]),
    # run-time shape: fewer samples than threads (16, 32), mixed radix (480 = 2^5 3 5; 192: its multiple of 64)
    ("rt16", 16, 16, {}, (16, 1, RT, 11), delays(16)),
    ("rt32", 32, 40, {}, (32, 2, RT, 11), [0, 31, 33, 3 * 32 + 5]),
    ("rt480", 480, 512, {}, (480, 2, RT, 11), delays(480, (192,))),
]

# the long delays again with runs of 1 and 3 blocks (option RUN): runs whose first block is not the call's first meet
# `tb * B < D`, in the workgroup forms and in the wave kernel (run: the option's value)
RUNS = [
    ("wave-512", 512, 512, {}, (512, 1, WAVE)),
    ("wave-1024", 1024, 512, {}, (512, 1, WAVE)),
    ("wg1024-k2wg", 512, 512, {"EARHIP_K2_WG": "1"}, (512, 1, WG)),
    ("wg2048-own", 1024, 512, {"EARHIP_K2_OWN_BLOCK": "1"}, (1024, 1, WG)),
    ("wg128", 64, 100, {}, (64, 2, WG)),
    ("wg512", 256, 512, {}, (256, 2, WG)),
]

# FIR lengths at the edges of the partition count, delay 2 B + 3: (B, n_taps, plan).  At block 512 the wave kernel gives way to
# the workgroup kernel with the second partition; at block 1024 the 513th tap ends the 512-sample partitions.
TAPS = [
    (64, 1, (64, 1, WG, 11)), (64, 63, (64, 1, WG, 11)), (64, 64, (64, 1, WG, 11)), (64, 65, (64, 2, WG, 11)), (64, 128, (64, 2, WG, 11)),
    (256, 1, (256, 1, WG, 11)), (256, 255, (256, 1, WG, 11)), (256, 256, (256, 1, WG, 11)), (256, 257, (256, 2, WG, 11)),
    (256, 512, (256, 2, WG, 11)),
    (512, 1, (512, 1, WAVE, 1)), (512, 511, (512, 1, WAVE, 1)), (512, 512, (512, 1, WAVE, 1)), (512, 513, (512, 2, WG, 11)),
    (512, 1024, (512, 2, WG, 11)),
    (480, 1, (480, 1, RT, 11)), (480, 479, (480, 1, RT, 11)), (480, 480, (480, 1, RT, 11)), (480, 481, (480, 2, RT, 11)),
    (480, 960, (480, 2, RT, 11)),
    (1024, 512, (512, 1, WAVE, 1)), (1024, 513, (1024, 1, WG, 7)), (1024, 2048, (1024, 2, WG, 7)),
]


def _plan(t):
    return dict(zip(("Bk", "NP", "form", "run"), t))


def _build():
    cases = []
    for group, B, n_taps, opts, plan, ds in FORMS:
        nb = NBLOCKS[B]
        for D in ds:
            cases.append(Case(f"{group}-d{D}", group, B, D, n_taps, nb, cuttings(nb), dict(opts), "0+5+0", _plan(plan)))
    for group, B, n_taps, opts, plan in RUNS:
        nb = NBLOCKS[B]
        for run in (1, 3):
            for D in (B + 1, 3 * B + 5):
                o = dict(opts, EARHIP_RUN=str(run))
                cases.append(Case(f"{group}-run{run}-d{D}", group, B, D, n_taps, nb, cuttings(nb), o, "0+5+0", _plan(plan + (run,))))
    for B, n_taps, plan in TAPS:
        nb = NBLOCKS[B]
        cases.append(Case(f"taps-b{B}-t{n_taps}", "taps", B, 2 * B + 3, n_taps, nb, cuttings(nb), {}, "0+5+0", _plan(plan)))
    # the wave kernel on 24 loudspeakers: several runs share a workgroup's spectrum in LDS, channel after channel
    cases.append(Case("wave-512-24ch-d1027", "wave-512", 512, 2 * 512 + 3, 512, 16, cuttings(16), {}, "9+10+3", _plan((512, 1, WAVE, 1))))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    for c in cases:
        assert c.nblocks <= 24 and c.nblocks * c.B <= 8192
        assert all(sum(cut) == c.nblocks for cut in c.cuttings)
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}
M_OBJECTS = 33  # (more than 32: the default gain kernels, with object splits on short calls)


def fir(n, n_taps):
    """512 taps: the product's own decorrelator design would do (scene()); any other length: seeded noise under a decaying
    envelope, as test_decorrelator_firs_longer_than_a_block makes them"""
    import numpy as np
    return (np.random.default_rng(n_taps).uniform(-1, 1, (n, n_taps)) * np.exp(-np.arange(n_taps) / 300.0)).astype(np.float32)


_scenes = {}


def scene(case, zero_diffuse=False):
    """(curves, inputs, FIRs, number of outputs) of a case — of its block size, length, FIR length and layout; the delay, the cutting
    and the options are the renderer's — made once and read-only.  zero_diffuse: every diffuse gain zero (the delay line alone)."""
    import numpy as np
    import scenes
    from layouts import LAYOUTS
    key = (case.B, case.nblocks, case.n_taps, case.layout, zero_diffuse)
    if key not in _scenes:
        n = len(LAYOUTS[case.layout])
        total = case.B * case.nblocks
        curves = scenes.adm_curves(M_OBJECTS, n, total, period=500, ramp=120, seed=case.B)
        if zero_diffuse:
            curves = [(t, d, np.zeros_like(f)) for t, d, f in curves]
        x = scenes.audio(M_OBJECTS, total, seed=case.B + 1)
        if case.n_taps == 512:
            from libear_amd import capi
            dec = capi.design_decorrelators(LAYOUTS[case.layout])
        else:
            dec = fir(n, case.n_taps)
        x.setflags(write=False)
        dec.setflags(write=False)
        _scenes[key] = (curves, x, dec, n)
    return _scenes[key]


def per_sample_over_rms(a, truth):
    """the worst difference of one sample divided by its channel's RMS in `truth`, over all channels"""
    import numpy as np
    a = np.asarray(a, np.float64)
    truth = np.asarray(truth, np.float64)
    rms = np.sqrt(np.mean(truth * truth, axis=1))
    assert np.all(rms > 0)
    return float(np.max(np.max(np.abs(a - truth), axis=1) / rms))


# The oracle's render against scenes.render_f64, per case: the worst per-sample difference over the channel's RMS, as
# tests/test_render_delay_cpu.py measured and printed it on its first run.  That test asserts them; the GPU test takes its
# per-sample bound from the largest.
ORACLE_PER_SAMPLE = {
    "wave-512-d0": 1.18e-06,  # (relative RMS 2.6e-07)
    "wave-512-d1": 1.15e-06,  # (relative RMS 2.55e-07)
    "wave-512-d511": 1.16e-06,  # (relative RMS 2.57e-07)
    "wave-512-d512": 1.27e-06,  # (relative RMS 2.55e-07)
    "wave-512-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wave-512-d1027": 1.28e-06,  # (relative RMS 2.56e-07)
    "wave-512-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wave-512-d63": 1.2e-06,  # (relative RMS 2.56e-07)
    "wave-512-d65": 1.32e-06,  # (relative RMS 2.52e-07)
    "wave-512-d256": 1.15e-06,  # (relative RMS 2.52e-07)
    "wave-512-d257": 1.19e-06,  # (relative RMS 2.47e-07)
    "wave-1024-d0": 1.13e-06,  # (relative RMS 2.56e-07)
    "wave-1024-d1": 1.11e-06,  # (relative RMS 2.55e-07)
    "wave-1024-d1023": 1.18e-06,  # (relative RMS 2.63e-07)
    "wave-1024-d1024": 1.15e-06,  # (relative RMS 2.58e-07)
    "wave-1024-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wave-1024-d2051": 1.19e-06,  # (relative RMS 2.66e-07)
    "wave-1024-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wave-1024-d511": 1.36e-06,  # (relative RMS 2.6e-07)
    "wave-1024-d513": 1.1e-06,  # (relative RMS 2.56e-07)
    "wave-2048-d0": 1.2e-06,  # (relative RMS 2.87e-07)
    "wave-2048-d513": 1.27e-06,  # (relative RMS 2.8e-07)
    "wave-2048-d2047": 1.47e-06,  # (relative RMS 2.9e-07)
    "wave-2048-d2049": 1.24e-06,  # (relative RMS 2.91e-07)
    "wave-2048-d6149": 1.47e-06,  # (relative RMS 3.37e-07)
    "wg1024-k2wg-d0": 1.18e-06,  # (relative RMS 2.6e-07)
    "wg1024-k2wg-d1": 1.15e-06,  # (relative RMS 2.55e-07)
    "wg1024-k2wg-d511": 1.16e-06,  # (relative RMS 2.57e-07)
    "wg1024-k2wg-d512": 1.27e-06,  # (relative RMS 2.55e-07)
    "wg1024-k2wg-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wg1024-k2wg-d1027": 1.28e-06,  # (relative RMS 2.56e-07)
    "wg1024-k2wg-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wg1024-513taps-d0": 1.51e-06,  # (relative RMS 3.27e-07)
    "wg1024-513taps-d511": 1.47e-06,  # (relative RMS 3.26e-07)
    "wg1024-513taps-d513": 1.47e-06,  # (relative RMS 3.25e-07)
    "wg1024-513taps-d1541": 1.44e-06,  # (relative RMS 3.26e-07)
    "wg2048-own-d0": 1.13e-06,  # (relative RMS 2.56e-07)
    "wg2048-own-d1": 1.11e-06,  # (relative RMS 2.55e-07)
    "wg2048-own-d1023": 1.18e-06,  # (relative RMS 2.63e-07)
    "wg2048-own-d1024": 1.15e-06,  # (relative RMS 2.58e-07)
    "wg2048-own-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wg2048-own-d2051": 1.19e-06,  # (relative RMS 2.66e-07)
    "wg2048-own-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wg2048-513taps-d0": 1.54e-06,  # (relative RMS 3.29e-07)
    "wg2048-513taps-d1023": 1.56e-06,  # (relative RMS 3.31e-07)
    "wg2048-513taps-d1025": 1.57e-06,  # (relative RMS 3.29e-07)
    "wg2048-513taps-d3077": 1.56e-06,  # (relative RMS 3.3e-07)
    "wg128-d0": 9.84e-07,  # (relative RMS 2.48e-07)
    "wg128-d1": 9.68e-07,  # (relative RMS 2.46e-07)
    "wg128-d63": 9.38e-07,  # (relative RMS 2.49e-07)
    "wg128-d64": 9.31e-07,  # (relative RMS 2.45e-07)
    "wg128-d65": 9.3e-07,  # (relative RMS 2.45e-07)
    "wg128-d131": 9.68e-07,  # (relative RMS 2.43e-07)
    "wg128-d197": 8.96e-07,  # (relative RMS 2.42e-07)
    "wg512-d0": 9.85e-07,  # (relative RMS 2.25e-07)
    "wg512-d1": 1.08e-06,  # (relative RMS 2.2e-07)
    "wg512-d255": 1.07e-06,  # (relative RMS 2.23e-07)
    "wg512-d256": 1.07e-06,  # (relative RMS 2.28e-07)
    "wg512-d257": 9.65e-07,  # (relative RMS 2.26e-07)
    "wg512-d515": 1.1e-06,  # (relative RMS 2.25e-07)
    "wg512-d773": 1.05e-06,  # (relative RMS 2.3e-07)
    "wg4096-own-d0": 1.2e-06,  # (relative RMS 2.87e-07)
    "wg4096-own-d2047": 1.47e-06,  # (relative RMS 2.9e-07)
    "wg4096-own-d2049": 1.24e-06,  # (relative RMS 2.91e-07)
    "wg4096-own-d6149": 1.47e-06,  # (relative RMS 3.37e-07)
    "rt16-d0": 6.93e-07,  # (relative RMS 1.98e-07)
    "rt16-d1": 7.42e-07,  # (relative RMS 2.12e-07)
    "rt16-d15": 6.49e-07,  # (relative RMS 1.85e-07)
    "rt16-d16": 6.24e-07,  # (relative RMS 1.93e-07)
    "rt16-d17": 6.87e-07,  # (relative RMS 1.95e-07)
    "rt16-d35": 7.52e-07,  # (relative RMS 2.02e-07)
    "rt16-d53": 6.37e-07,  # (relative RMS 1.97e-07)
    "rt32-d0": 1e-06,  # (relative RMS 2.43e-07)
    "rt32-d31": 1.07e-06,  # (relative RMS 2.45e-07)
    "rt32-d33": 1.09e-06,  # (relative RMS 2.5e-07)
    "rt32-d101": 9.73e-07,  # (relative RMS 2.4e-07)
    "rt480-d0": 1.37e-06,  # (relative RMS 2.91e-07)
    "rt480-d1": 1.44e-06,  # (relative RMS 2.88e-07)
    "rt480-d479": 1.41e-06,  # (relative RMS 2.87e-07)
    "rt480-d480": 1.3e-06,  # (relative RMS 2.87e-07)
    "rt480-d481": 1.32e-06,  # (relative RMS 2.82e-07)
    "rt480-d963": 1.26e-06,  # (relative RMS 2.92e-07)
    "rt480-d1445": 1.33e-06,  # (relative RMS 2.93e-07)
    "rt480-d192": 1.43e-06,  # (relative RMS 2.79e-07)
    "wave-512-run1-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wave-512-run1-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wave-512-run3-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wave-512-run3-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wave-1024-run1-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wave-1024-run1-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wave-1024-run3-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wave-1024-run3-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wg1024-k2wg-run1-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wg1024-k2wg-run1-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wg1024-k2wg-run3-d513": 1.16e-06,  # (relative RMS 2.52e-07)
    "wg1024-k2wg-run3-d1541": 1.22e-06,  # (relative RMS 2.61e-07)
    "wg2048-own-run1-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wg2048-own-run1-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wg2048-own-run3-d1025": 1.17e-06,  # (relative RMS 2.6e-07)
    "wg2048-own-run3-d3077": 1.23e-06,  # (relative RMS 2.75e-07)
    "wg128-run1-d65": 9.3e-07,  # (relative RMS 2.45e-07)
    "wg128-run1-d197": 8.96e-07,  # (relative RMS 2.42e-07)
    "wg128-run3-d65": 9.3e-07,  # (relative RMS 2.45e-07)
    "wg128-run3-d197": 8.96e-07,  # (relative RMS 2.42e-07)
    "wg512-run1-d257": 9.65e-07,  # (relative RMS 2.26e-07)
    "wg512-run1-d773": 1.05e-06,  # (relative RMS 2.3e-07)
    "wg512-run3-d257": 9.65e-07,  # (relative RMS 2.26e-07)
    "wg512-run3-d773": 1.05e-06,  # (relative RMS 2.3e-07)
    "taps-b64-t1": 8.5e-07,  # (relative RMS 1.61e-07)
    "taps-b64-t63": 8.93e-07,  # (relative RMS 2.44e-07)
    "taps-b64-t64": 1.05e-06,  # (relative RMS 2.44e-07)
    "taps-b64-t65": 1.03e-06,  # (relative RMS 2.49e-07)
    "taps-b64-t128": 1e-06,  # (relative RMS 2.45e-07)
    "taps-b256-t1": 1.06e-06,  # (relative RMS 1.71e-07)
    "taps-b256-t255": 1.2e-06,  # (relative RMS 3e-07)
    "taps-b256-t256": 1.23e-06,  # (relative RMS 2.88e-07)
    "taps-b256-t257": 1.41e-06,  # (relative RMS 2.94e-07)
    "taps-b256-t512": 1.1e-06,  # (relative RMS 2.25e-07)
    "taps-b512-t1": 9.56e-07,  # (relative RMS 1.86e-07)
    "taps-b512-t511": 1.48e-06,  # (relative RMS 3.25e-07)
    "taps-b512-t512": 1.28e-06,  # (relative RMS 2.56e-07)
    "taps-b512-t513": 1.45e-06,  # (relative RMS 3.26e-07)
    "taps-b512-t1024": 1.47e-06,  # (relative RMS 3.22e-07)
    "taps-b480-t1": 9.24e-07,  # (relative RMS 2.08e-07)
    "taps-b480-t479": 1.56e-06,  # (relative RMS 3.74e-07)
    "taps-b480-t480": 1.73e-06,  # (relative RMS 3.78e-07)
    "taps-b480-t481": 1.88e-06,  # (relative RMS 3.62e-07)
    "taps-b480-t960": 1.96e-06,  # (relative RMS 3.68e-07)
    "taps-b1024-t512": 1.19e-06,  # (relative RMS 2.66e-07)
    "taps-b1024-t513": 1.53e-06,  # (relative RMS 3.3e-07)
    "taps-b1024-t2048": 1.44e-06,  # (relative RMS 3.29e-07)
    "wave-512-24ch-d1027": 1.17e-06,  # (relative RMS 2.63e-07)
}
