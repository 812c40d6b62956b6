"""CPU tests of the multi-GPU launch path: pythtb_amd/launch.py, and `python bench.py --gpus N` starting its own ranks
(VERDICT r2 item 1).  `--stub` replaces the GPU step by a no-op so that the whole control flow -- launcher, gloo
rendezvous, barriers around the timed loop, communicator-first gather, fallback labelling, exit status -- runs here."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, OMP_NUM_THREADS="1", TBK_BENCH_RCCL_TIMEOUT="60")
ENV.pop("WORLD_SIZE", None)
ENV.pop("RANK", None)

WORKER = r"""
import os, sys, time
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert os.environ["LOCAL_RANK"] == os.environ["RANK"] and os.environ["MASTER_ADDR"] == "127.0.0.1"
mode = sys.argv[1]
if mode == "ok":
    import torch, torch.distributed as dist
    dist.init_process_group("gloo")
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t)
    if rank == 0:
        print("SUM", int(t.item()), world, flush=True)
    dist.destroy_process_group()
elif mode == "fail":
    if rank == 1:
        sys.exit(7)
    time.sleep(600)          # the surviving ranks would wait for ever: the launcher must end them
"""


def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tbk_launch_t", os.path.join(ROOT, "pythtb_amd", "launch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launcher_module_loads_without_the_library():
    """bench.py loads launch.py by path, before anything GPU-side: it must import nothing but the standard library."""
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('l', %r); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); assert 'pythtb_amd' not in sys.modules and 'torch' not in sys.modules "
            "and 'numpy' not in sys.modules; print('OK')" % os.path.join(ROOT, "pythtb_amd", "launch.py"))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "OK" in res.stdout, res.stderr


def test_spawn_ranks_runs_a_gloo_job_and_relays_output(tmp_path, capfd):
    pytest.importorskip("torch")
    w = tmp_path / "w.py"
    w.write_text(WORKER)
    rc = _launcher().spawn_ranks(str(w), ["ok"], 3, env=ENV, timeout=300)
    out = capfd.readouterr().out
    assert rc == 0 and "SUM 6 3" in out


def test_spawn_ranks_ends_the_survivors_when_one_rank_fails(tmp_path):
    w = tmp_path / "w.py"
    w.write_text(WORKER)
    t0 = time.monotonic()
    rc = _launcher().spawn_ranks(str(w), ["fail"], 3, env=ENV, timeout=300)
    assert rc == 7 and time.monotonic() - t0 < 60


def _bench(args, env=ENV, prefix=()):
    cmd = list(prefix) + [os.path.join(ROOT, "bench.py")] + args
    res = subprocess.run([sys.executable] + cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    return res, lines


@pytest.mark.parametrize("world", [2, 3, 8])
def test_bench_starts_its_own_ranks(world):
    """`python bench.py --gpus N` with WORLD_SIZE unset (how the driver runs N = 1) must not die at argument parsing."""
    pytest.importorskip("torch")
    res, lines = _bench(["--gpus", str(world), "--steps", "4", "--warmup", "1", "--stub"])
    assert res.returncode == 0, res.stderr[-3000:]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == world and out["steps"] == 4 and out["scaling"] == "weak"
    assert out["config"]["gather"] == "stub_allgather" and out["config"]["global_mesh"] == [2048 * world, 2048]
    assert abs(out["check"]["chern"] + 1.0) < 1e-12 and out["check"]["min_gap"] == 1.5
    assert abs(out["value"] - 2048 * 2048 * world * 4 / (out["ms_per_step"] * 4e-3)) < 1e-6 * out["value"]


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) times the headline only and says so; --dump-outputs DIR writes every rank's last-step
    results as float64 .npy files, the same from run to run."""
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        res, lines = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--stub", "--dump-outputs", str(d)])
        assert res.returncode == 0, res.stderr[-3000:]
        out = json.loads(lines[0])
        assert out["full"] is False and out["steps"] == 3 and out["ms_per_step"] > 0
        for leg in ("cpu_baseline", "sustained", "fused_extension", "python_api", "configs", "cold_burst"):
            assert leg not in out, leg
        names = sorted(os.listdir(str(d)))
        assert names == ["rank%d_%s.npy" % (r, n) for r in (0, 1) for n in ("berry_flux", "min_gaps")], names
        arrs = {n: np.load(str(d / n)) for n in names}
        assert all(a.dtype == np.float64 for a in arrs.values())
        outs.append(arrs)
    assert all(np.array_equal(outs[0][n], outs[1][n]) for n in outs[0])
    assert abs(outs[0]["rank0_berry_flux.npy"][0] + outs[0]["rank1_berry_flux.npy"][0] + 2 * np.pi) < 1e-12


def test_bench_multi_rank_control_flow_needs_no_torch(tmp_path):
    """VERDICT r5 #8 / north_star "no PyTorch": `bench.py --gpus 2` with torch made un-importable in the launcher AND in
    every rank (sys.modules['torch'] = None): the ranks meet on the launcher's TCP rendezvous (launch.Rendezvous), hand
    round the communicator id, agree, gather -- the stub communicator's path and the labelled fallback alike."""
    shim = tmp_path / "bench_no_torch.py"
    shim.write_text("import sys\nsys.modules['torch'] = None\nimport runpy\nsys.argv[0] = %r\n"
                    "runpy.run_path(sys.argv[0], run_name='__main__')\n" % os.path.join(ROOT, "bench.py"))
    # (bench.py re-launches `os.path.abspath(__file__)` for its ranks: give it the shim as its own file name)
    env = dict(ENV, TBK_BENCH_SELF=str(shim))
    for extra, rc, gather in (({}, 0, "stub_allgather"), ({"TBK_BENCH_STUB_COMM": "fail"}, 4, "socket (FALLBACK: rccl")):
        res = subprocess.run([sys.executable, str(shim), "--gpus", "2", "--steps", "3", "--warmup", "1", "--stub"],
                             env=dict(env, **extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert res.returncode == rc, (res.returncode, res.stderr[-3000:])
        assert len(lines) == 1, res.stdout
        out = json.loads(lines[0])
        assert out["n_gpus"] == 2 and out["config"]["gather"].startswith(gather) and abs(out["check"]["chern"] + 1.0) < 1e-12


def test_rendezvous_operations_and_stale_files(tmp_path):
    """launch.Rendezvous on three ranks (threads here): all-gather of byte strings in rank order, broadcast, all_min,
    barriers; rank 0's port file is removed at close; a stale file of an earlier run (nobody listening / wrong token) is
    skipped, not believed."""
    import threading
    L = _launcher()
    port = L.free_port()
    out, errs = {}, []

    def run(r, busy):
        try:
            z = L.Rendezvous(rank=r, world=3, addr="127.0.0.1", port=port, timeout=30)
            z.barrier()
            g = z.allgather_bytes(b"x" * r)
            b = z.broadcast_bytes(b"id-of-128-bytes" if r == 1 else None, src=1)
            m = z.all_min(5 - r)
            out[(busy, r)] = (g, b, m, z._rdzv_file())
            z.barrier()
            z.close()
        except Exception as e:                          # noqa: BLE001
            errs.append(e)
    for busy in (False, True):
        hold = None
        if busy:                                        # MASTER_PORT taken (torch.distributed.run's store) + a stale file
            import socket
            hold = socket.socket()
            hold.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)      # (the first round's connections sit in TIME_WAIT)
            hold.bind(("127.0.0.1", port))
            hold.listen(1)
            with open(out[(False, 0)][3], "w") as f:
                json.dump({"port": L.free_port(), "token": "0" * 32, "pid": 1}, f)
        ts = [threading.Thread(target=run, args=(r, busy)) for r in (1, 2, 0)]
        for t in ts:
            t.start()
            time.sleep(0.2)
        for t in ts:
            t.join(60)
        if hold is not None:
            hold.close()
        assert not errs, errs
        for r in range(3):
            g, b, m, path = out[(busy, r)]
            assert g == [b"", b"x", b"xx"] and b == b"id-of-128-bytes" and m == 3
        assert not os.path.exists(out[(busy, 0)][3])


def test_bench_same_behaviour_under_torch_distributed_run():
    pytest.importorskip("torch")
    port = _launcher().free_port()
    res, lines = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--stub"],
                        prefix=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                "--master-addr", "127.0.0.1", "--master-port", str(port)])
    assert res.returncode == 0, res.stderr[-3000:]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2


def test_bench_reports_a_failed_communicator_as_failure_with_the_line_still_printed():
    pytest.importorskip("torch")
    res, lines = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--stub"], env=dict(ENV, TBK_BENCH_STUB_COMM="fail"))
    assert res.returncode == 4, (res.returncode, res.stderr[-2000:])
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["config"]["gather"].startswith("socket (FALLBACK: rccl") and abs(out["check"]["chern"] + 1.0) < 1e-12
    # the optional gloo rendezvous (rounds 2-5) keeps working and labels itself
    res, lines = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--stub"],
                        env=dict(ENV, TBK_BENCH_STUB_COMM="fail", TBK_RENDEZVOUS="gloo"))
    assert res.returncode == 4 and json.loads(lines[0])["config"]["gather"].startswith("gloo (FALLBACK: rccl")


def test_bench_without_a_gpu_fails_in_the_ranks_not_at_launch():
    """No GPU here: the two children must get as far as creating their context ("no HIP device"), and the launcher must
    return their failure."""
    res, lines = _bench(["--gpus", "2", "--steps", "2"])
    assert res.returncode != 0 and not lines
    assert "no HIP device is visible" in res.stderr and "must be launched with" not in res.stderr
