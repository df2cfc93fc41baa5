"""The multi-GPU plumbing of bench.py and deequ_amd.distributed (AnalysisRunner.scala:303's partial ->
final merge across ranks), executed for real:

* CPU: `bench.py --gpus N` re-launches itself as N ranks through torch.distributed.run before anything
  touches the GPU (the command it builds);
* GPU: two ranks sharing the box's one GPU run the whole bench (scan, all-gather + rank-order combine,
  StateLoader append) over gloo and print ONE line with n_gpus = 2 and a measured merge time;
* GPU: a world-size-1 "nccl" (RCCL) process group initialised with device_id exactly as bench.py does,
  so allgather_combine's device-tensor branch runs (RCCL needs distinct GPUs per rank, so one rank is
  what a one-GPU box can run);
* the plain / `--full` split of bench.py's options and `--dump-outputs` (CPU: hand-made slot sets; GPU: a small
  plain run twice, the same arrays both times).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def test_bench_launcher_builds_torchrun_command(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert bench.launch_ranks(bench.parse(["--gpus", "4", "--steps", "3"])) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_full_is_off_by_default_and_skip_headline_needs_it():
    sys.path.insert(0, ROOT)
    import bench

    args = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    assert bench.parse(["--full", "--skip-headline", "--configs", "c3"]).full is True
    with pytest.raises(SystemExit):
        bench.parse(["--skip-headline", "--configs", "c3"])
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_bench_dump_outputs_arrays(tmp_path):
    """dump_outputs on hand-made slot sets: metrics in analyzer order (NaN for an empty state), the non-HLL
    fields as float64, the HLL words as exact 16-bit quarters in float32."""
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench
    import deequ_amd as dq
    from deequ_amd import _lib as L
    from deequ_amd.states import (ApproxCountDistinctState, MeanState, NumMatches, NumMatchesAndCount, state_to_c)

    words = tuple([(1 << 62) + 3] + [0] * 50 + [-1])
    empty = L.State()
    empty.op = L.OP_MIN
    analyzers = [dq.Size(), dq.Mean("c"), dq.ApproxCountDistinct("c"), dq.Completeness("c"), dq.Minimum("c")]
    states = [state_to_c(NumMatches(10), L.OP_SIZE), state_to_c(MeanState(5.0, 2), L.OP_MEAN),
              state_to_c(ApproxCountDistinctState(words), L.OP_APPROX_COUNT_DISTINCT),
              state_to_c(NumMatchesAndCount(3, 4), L.OP_COMPLETENESS), empty]
    bench.dump_outputs(str(tmp_path / "out"), analyzers, states)
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("metrics", "state_fields", "hll_words")}
    assert got["metrics"].dtype == np.float64 and got["state_fields"].dtype == np.float64
    assert got["hll_words"].dtype == np.float32 and got["hll_words"].shape == (1, 52 * 4)
    m = got["metrics"]
    assert m[0] == 10.0 and m[1] == 2.5 and m[3] == 0.75 and np.isnan(m[4]) and m[2] > 0.0
    assert got["state_fields"].tolist() == [10.0, 5.0, 2.0, 3.0, 4.0]
    back = got["hll_words"].astype(np.uint16).view(np.int64).reshape(-1)
    assert tuple(int(w) for w in back) == words


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain run prints the headline line alone and --dump-outputs writes the last timed step's outputs:
    the same arrays from two runs, Size = rows x (warm-up + timed steps) after the incremental append."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "200003", "--chunk", "100000",
               "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / name)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        rec = json.loads(lines[0])
        assert rec["steps"] == 2 and rec["ms_per_step"] > 0.0 and rec["unit"] == "rows/s"
        assert abs(rec["value"] - 200003 / (rec["ms_per_step"] * 1e-3)) <= 1e-9 * rec["value"]
        for moved in ("roofline", "configs", "cpu_baseline", "ingest", "state_io", "plan_create_ms"):
            assert moved not in rec
        dumps.append({n: np.load(tmp_path / name / f"{n}.npy") for n in ("metrics", "state_fields", "hll_words")})
    a, b = dumps
    assert a["metrics"].shape == (93,) and a["hll_words"].shape == (16, 208)
    assert a["metrics"][0] == 200003 * 3 and not np.isnan(a["metrics"]).any()
    for n in a:
        assert a[n].tobytes() == b[n].tobytes(), n


@pytest.mark.gpu
def test_bench_two_ranks_gloo_on_one_gpu():
    env = dict(os.environ)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--rows",
           "4000000", "--chunk", "2000000", "--steps", "2", "--warmup", "1", "--configs", "", "--cpu-sample", "0",
           "--ingest-rows", "0"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    assert rec["rank_merge_ms_per_step"] > 0.0
    assert rec["value"] > 0 and rec["config"]["rows_per_gpu"] == 4_000_000


def _nccl_worker(port, q):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    assert dist.get_backend() == "nccl"
    from deequ_amd import distributed, synth
    from deequ_amd.runner import scan_results
    from deequ_amd.states import state_from_c

    t = synth.c5_table(100_000, seed=21)
    analyzers = synth.profile_analyzers(t)
    res = scan_results(t, analyzers)
    merged = distributed.allgather_combine(res)  # device tensors through RCCL
    q.put(([repr(state_from_c(s)) for s in res], [repr(state_from_c(s)) for s in merged]))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_nccl_world_size_one_allgather_combine():
    import torch.multiprocessing as mp

    from tests.test_distributed import _free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(_free_port(), q))
    p.start()
    before, after = q.get(timeout=180)
    p.join(60)
    assert p.exitcode == 0
    assert before == after  # one rank: the all-gather + combine is the identity on the slot set
