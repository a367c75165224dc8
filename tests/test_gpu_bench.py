"""bench.py itself, at reduced stream lengths: a plain run prints the headline line alone, every BASELINE configuration
produces a complete --full line (roofline + cpu_baseline + parity on the timed output, per channel), and the multi-rank control flow
(object sharding, ragged channel ownership, the exchange, the self-check) runs with several ranks
sharing the one GPU of the box over gloo.  Each run is a fresh child process (torchrun for N > 1)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    """a port nobody listens on, taken BELOW the kernel's ephemeral range (32768-60999): a port from that range (bind to 0) can be
    handed to somebody's outgoing connection between this check and the rendezvous' own bind (seen once: EADDRINUSE)"""
    import random
    for _ in range(64):
        port = random.randint(15000, 30000)
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", port))
        except OSError:
            continue
        finally:
            s.close()
        return port
    raise RuntimeError("no free port found")


def _run_with_one_retry(cmd, env, timeout):
    """Several ranks sharing ONE GPU over gloo (the functional check of the multi-rank control flow on a one-GPU box) hung
    once in some dozens of runs — both ranks alive, no progress, nothing in their output — and ran through when started
    again; a rendezvous over TCP between processes that time-slice one device is not what is under test here.  So:
    a bounded wait and one second try; a second hang fails the test."""
    import signal
    for attempt in (0, 1):
        # (its own process group: on a timeout the launcher AND the ranks it started are ended, by that group's id)
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT, start_new_session=True)
        try:
            out, err = proc.communicate(timeout=timeout)
            if attempt == 0 and proc.returncode != 0 and "EADDRINUSE" in err and "--master-port" in cmd:
                cmd = list(cmd)  # somebody took the rendezvous port between the check and the bind: once more on another one
                cmd[cmd.index("--master-port") + 1] = str(_free_port())
                continue
            return subprocess.CompletedProcess(cmd, proc.returncode, out, err)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            proc.communicate()
            if attempt == 1:
                raise
            if "--master-port" in cmd:  # a fresh port for the second try
                cmd = list(cmd)
                cmd[cmd.index("--master-port") + 1] = str(_free_port())


def run_bench(args, nproc=1, env=None):
    cmd = [sys.executable]
    if nproc > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
                "127.0.0.1", "--master-port", str(_free_port())]
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + args
    e = dict(os.environ)
    e.update(env or {})
    res = _run_with_one_retry(cmd, e, 900 if nproc == 1 else 300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone(tmp_path):
    """without --full a run times its steps, writes --dump-outputs and prints the headline fields; none of the legs that
    --full adds (parity gate, CPU baseline, other precisions, block mode, host-pointer calls, per-step events, the read
    bandwidth probe, the secondary workloads) runs"""
    import numpy as np
    line = run_bench(["--blocks", "64", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["metric"] == "Msamples/s" and line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 4 and line["dtype"].startswith("f32")
    assert line["kernels_ms"]["gain_mix"] > 0 and line["roofline"]["peak_measured"] is None
    moved = {"parity", "cpu_baseline", "value_f32_exact", "value_strict", "block_mode", "host_stream", "step_ms", "secondary"}
    assert not moved & set(line), sorted(moved & set(line))
    out = np.load(tmp_path / "outputs.npy")
    assert out.shape == (line["config"]["channels"], 64 * line["config"]["block"]) and np.isfinite(out).all()


@pytest.mark.parametrize("config", ["C2", "C3", "C4", "C5"])
def test_every_baseline_config_gives_a_complete_parity_checked_line(config):
    line = run_bench(["--full", "--config", config, "--blocks", "64", "--steps", "4", "--warmup", "1", "--cpu-blocks", "4"])
    assert line["metric"] == "Msamples/s" and line["n_gpus"] == 1 and line["value"] > 0
    assert line["config"]["baseline_config"] == config
    assert line["dtype"].startswith("f32")
    r = line["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1.0 and r["peak"] == 8000.0
    assert r["traffic"] is None or r["traffic_source"]
    assert r["peak_measured"] and "error" not in r["peak_measured"]
    p = line["parity"]
    assert p["same_plan_as_timed"]
    assert p["pass"] and p["rel_rms_vs_cpu"] <= 1e-6 and p["max_channel_rel_rms_vs_cpu"] <= 1e-6
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["cpu_model"]
    assert line["value_f32_exact"]["value"] > 0 and line["value_strict"]["value"] > 0
    assert line["step_ms"]["median"] > 0 and line["block_mode"]["ms_per_block"] > 0


def test_one_gpu_line_is_the_same_measurement_with_or_without_a_shard_mode():
    """`--gpus 1 --shard objects` is the plain one-GPU line: the same workload, launch plan and parity gate, no exchange object,
    and the same figure up to run-to-run noise (a first multi-GPU contact reads its N = 1 point against the headline)."""
    common = ["--full", "--blocks", "256", "--steps", "8", "--warmup", "2", "--cpu-blocks", "0", "--brief"]
    plain = run_bench(common)
    sharded = run_bench(["--shard", "objects"] + common)
    for line in (plain, sharded):
        assert line["n_gpus"] == 1 and line["exchange"] is None and line["config"]["shard"] is None
        assert line["parity"]["pass"]
    assert plain["config"]["workload"] == sharded["config"]["workload"]
    assert plain["roofline"]["plan"] == sharded["roofline"]["plan"] and plain["roofline"]["kernel"] == sharded["roofline"]["kernel"]
    assert 0.8 <= sharded["value"] / plain["value"] <= 1.25, (plain["value"], sharded["value"])


def test_default_invocation_measures_libears_own_calling_convention():
    """the host-pointer stream calls (earhip_render_process from pageable and from device-reachable rows, 64 blocks per call here)
    are part of the --full line: rate, the measured H2D rate beside it, and their outputs held against the device-resident render"""
    line = run_bench(["--full", "--blocks", "64", "--steps", "4", "--warmup", "1", "--cpu-blocks", "4", "--no-secondary"])
    hs = line["host_stream"]
    assert hs["pass"] and hs["h2d_GBps_measured"]["pinned"] > 1.0
    srcs = {(c["source"], c["blocks_per_call"]) for c in hs["calls"]}
    assert srcs == {("pageable", 64), ("pinned", 64)}, srcs
    for c in hs["calls"]:
        assert c["Gsamples_per_s"] > 0 and 0 < c["frac"] < 1.2 and c["max_channel_rel_rms_vs_cpu"] <= 1e-6, c


@pytest.mark.parametrize("scene,kernel,tile", [("adm", "k_gain_mix_p2", 512), ("moving", "k_gain_mix_hg", 512),
                                               ("mixed", "k_gain_mix_h2", 512), ("panned-adm", "k_gain_mix_p2", 512)])
def test_scenes_at_the_headline_size_pass_the_parity_gate_of_their_own_launch_plan(scene, kernel, tile):
    """1024 objects x 512 blocks: the calls long enough for the launch plans only long calls get (the piece-list
    kernel's paired lists on 8-wave, 512-sample tiles for ADM-like metadata, the hinge kernel on 512 for curves that
    ramp all the time; a ramp that starts on a tile's last sample was lost there once) — the parity gate compares the
    timed call's own output with the CPU path, per channel"""
    forced = any(os.environ.get(k) is not None for k in ("EARHIP_P2_PAIRS", "EARHIP_P2_TILE", "EARHIP_H2_TILE", "EARHIP_MFMA", "EARHIP_HINGE", "EARHIP_HG_TILE"))
    if forced and scene == "moving" and os.environ.get("EARHIP_P2_PAIRS") == "1":
        pytest.skip("paired lists forced onto always-ramping curves: not the layout the library picks for them (its pair "
                    "chunks do not sum per chunk: 1.0e-6 from the CPU path at this size)")
    line = run_bench(["--full", "--scene", scene, "--blocks", "512", "--steps", "2", "--warmup", "1", "--cpu-blocks", "0"])
    if not forced:
        assert kernel in line["roofline"]["kernel"], line["roofline"]["kernel"]
        assert line["roofline"]["plan"]["tile_samples"] == tile, line["roofline"]["plan"]
    p = line["parity"]
    assert p["same_plan_as_timed"] and p["pass"], p
    assert p["max_channel_rel_rms_vs_cpu"] <= 1e-6


@pytest.mark.parametrize("nproc,layout", [(2, "9+10+3"), (3, "4+5+0")])
def test_multi_rank_control_flow_on_one_gpu_over_gloo(nproc, layout):
    """ranks share cuda:0, the collective runs over gloo: sharding, ragged channel ownership (10 channels
    over 3 ranks), the asynchronous exchange and its self-check (owned slice == all-reduce of the partials)"""
    line = run_bench(["--full", "--objects", "96", "--layout", layout, "--blocks", "32", "--steps", "3", "--warmup", "1",
                      "--cpu-blocks", "0"], nproc=nproc,
                     env={"EARHIP_BENCH_BACKEND": "gloo", "EARHIP_BENCH_CHECK": "force"})
    assert line["n_gpus"] == nproc and line["scaling"] == "strong"
    assert line["config"]["objects_total"] == 96 and line["config"]["objects_per_gpu"] == 96 // nproc
    assert line["exchange_check"]["max_rel_err_owned_slice_vs_all_reduce"] <= 1e-6
    assert line["weak_scaling"]["objects_total"] == 96 * nproc and line["weak_scaling"]["value"] > 0
    if 32 % nproc == 0:  # the same line measures the other two decompositions (short runs)
        assert set(line["other_shard_modes"]) == {"objects-nogather", "time"}
        assert all(m["value"] > 0 for m in line["other_shard_modes"].values())
        assert line["other_shard_modes"]["time"]["objects_per_gpu"] == 96


@pytest.mark.parametrize("nproc", [2, 3])
def test_time_sharding_on_one_gpu_over_gloo(nproc):
    """--shard time: every rank renders ALL objects for its T / G blocks behind one lead block; no exchange.  The line's
    own check: a rank's blocks after one lead block are bit-identical to the same blocks after three."""
    line = run_bench(["--full", "--objects", "96", "--blocks", "48", "--steps", "3", "--warmup", "1", "--cpu-blocks", "0", "--shard", "time"],
                     nproc=nproc, env={"EARHIP_BENCH_BACKEND": "gloo"})
    assert line["n_gpus"] == nproc and line["config"]["shard"] == "time"
    assert line["config"]["objects_total"] == 96 and line["config"]["objects_per_gpu"] == 96
    assert line["exchange"]["mode"] == "time" and line["exchange"]["reduce_scatter_bytes_per_rank"] == 0
    assert line["exchange"]["blocks_of_this_rank"] == [0, 48 // nproc]
    assert line["exchange"]["model"]["exchange_ms_per_step"] == 0
    assert line["exchange_check"]["max_rel_diff_one_lead_block_vs_three"] <= 1e-6
    assert "time-sharded" in line["config"]["parallelism"]


def test_objects_without_gather_on_one_gpu_over_gloo():
    """--shard objects-nogather: the reduce-scatter alone (the consumer takes the bus channel-sharded); the exchange
    model counts one slice instead of two; the same partials exchanged twice give bit-identical slices"""
    line = run_bench(["--full", "--objects", "96", "--blocks", "32", "--steps", "3", "--warmup", "1", "--cpu-blocks", "0",
                      "--shard", "objects-nogather"], nproc=2, env={"EARHIP_BENCH_BACKEND": "gloo", "EARHIP_BENCH_CHECK": "force"})
    assert line["config"]["shard"] == "objects-nogather"
    assert line["exchange"]["gather_bytes_into_root"] == 0 and line["exchange"]["root"] is None
    assert line["exchange"]["reduce_scatter_bytes_per_rank"] == 12 * 32 * 512 * 4
    assert line["exchange_check"]["max_rel_err_owned_slice_vs_all_reduce"] <= 1e-6
    assert line["exchange_check"]["same_partials_exchanged_twice_bit_identical"] is True
    m = line["exchange"]["model"]
    assert m["mode"] == "objects-nogather" and "unmeasured" in m["status"]


def test_plain_invocation_with_gpus_2_launches_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` exactly as the driver runs the N = 1 command, no launcher around it: bench.py
    starts its ranks itself (a fresh torchrun child) and relays rank 0's line.  On a one-GPU box the two ranks share
    the device and the exchange runs over gloo (said in config.parallelism); on a multi-GPU node the same command
    runs one rank per GPU on libearhip's own RCCL communicator."""
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e["EARHIP_BENCH_CHECK"] = "force"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--objects", "128", "--blocks", "32", "--steps", "3",
           "--warmup", "1", "--cpu-blocks", "0"]
    res = _run_with_one_retry(cmd, e, 300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["objects_per_gpu"] == 64
    import torch
    if torch.cuda.device_count() < 2:
        assert "ranks share GPUs" in line["config"]["parallelism"]
    else:
        assert "earhip_comm" in line["config"]["parallelism"]
        assert line["exchange"]["collectives_ms"] > 0
    assert line["exchange"]["reduce_scatter_bytes_per_rank"] == 12 * 32 * 512 * 4
    assert line["exchange_check"]["max_rel_err_owned_slice_vs_all_reduce"] <= 1e-6


def test_refbench_line():
    """bench.py --config refbench: the reference's own benchmark shape (32 -> 24 channels, 1024 samples, a matrix point
    every 100 samples) in block and stream mode with the CPU path beside it, parity-gated"""
    line = run_bench(["--full", "--config", "refbench", "--steps", "5", "--warmup", "2"])
    assert line["config"]["baseline_config"] == "refbench" and line["value"] > 0
    assert line["block_mode"]["ms_per_call"] > 0 and line["cpu_baseline"]["ms_per_call"] > 0
    assert line["parity"]["pass"] and line["parity"]["block_rel_rms_vs_cpu"] <= 1e-6
    assert len(line["crossover"]["sweep_24_outputs_1024_samples"]) == 8


def test_producer_line():
    """bench.py --producer: the Objects gain producer with extent through device pointers, parity-gated"""
    line = run_bench(["--full", "--producer", "20000", "--steps", "3", "--warmup", "1"])
    assert line["unit"] == "Mpositions/s" and line["value"] > 0
    assert line["parity"]["pass"] and line["parity"]["max_rel_norm"] <= 1e-5
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"


def test_default_line_carries_the_other_workloads():
    """`python bench.py --full` (fewer steps here): the headline line carries a `secondary` array — the other
    BASELINE configurations and the scenes of the other gain kernels, each timed in a process of its own with the parity gate
    on its own timed buffer"""
    if any(os.environ.get(k) is not None for k in ("EARHIP_P2_PAIRS", "EARHIP_P2_TILE", "EARHIP_H2_TILE", "EARHIP_MFMA", "EARHIP_HINGE", "EARHIP_HG_TILE")):
        pytest.skip("kernel forced")
    line = run_bench(["--full", "--steps", "6", "--warmup", "2", "--cpu-blocks", "4"])
    sec = {e["workload"]: e for e in line["secondary"]}
    assert {"C2", "C3", "C5", "C4 adm", "C4 moving", "C4 bursty"} <= set(sec), sorted(sec)
    for name, e in sec.items():
        assert "error" not in e, (name, e.get("error"))
        assert e["value"] > 0 and e["steps"] >= 5 and 0 < e["roofline"]["frac"] < 1.0, (name, e)
        assert e["parity"]["pass"] and e["parity"]["same_plan_as_timed"] and e["parity"]["max_channel_rel_rms_vs_cpu"] <= 1e-6, (name, e)
    assert "k_gain_mix_hg" in sec["C4 moving"]["roofline"]["kernel"] and "k_gain_mix_p2" in sec["C4 adm"]["roofline"]["kernel"]
    assert "k_gain_mix_h2" in sec["C4 bursty"]["roofline"]["kernel"]


def test_dump_outputs_writes_the_last_timed_step_and_repeats(tmp_path):
    """--dump-outputs DIR: the loudspeaker outputs of the last timed step as DIR/outputs.npy (float32, [channels][samples]); the
    same arguments give the same inputs, so a second run writes the same outputs; --steps is the number of timed steps"""
    import numpy as np
    common = ["--full", "--blocks", "64", "--steps", "5", "--warmup", "1", "--cpu-blocks", "0", "--brief"]
    got = []
    for run in ("a", "b"):
        line = run_bench(common + ["--dump-outputs", str(tmp_path / run)])
        assert line["steps"] == 5 and line["parity"]["pass"]
        out = np.load(tmp_path / run / "outputs.npy")
        assert out.dtype == np.float32 and out.shape == (line["config"]["channels"], 64 * line["config"]["block"])
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        got.append(out)
    assert np.linalg.norm(got[0] - got[1]) <= 1e-6 * np.linalg.norm(got[1])
