"""bench.py end to end on the GPU box, at sizes that take seconds: the default line's contract (one JSON line on stdout, the
roofline / cpu_baseline objects) on the small BASELINE configuration, what --dump-outputs writes and what --full adds, and
the one-GPU rehearsal of a rank of an N-GPU job over a real RCCL communicator."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MIMI_BENCH_BACKEND")}
    env.update(extra_env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[:2000]            # stdout carries the one JSON line and nothing else
    return json.loads(lines[0])


def test_bench_line_contract_on_the_small_configuration():
    d = run_bench("--workload", "cfg2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f64" and d["config"]["name"] == "cfg2"
    assert d["config"]["kernel_path"] == "tensor"
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and 0.0 < roof["frac"] < 1.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12
    # whole-job rate = elements x steps / time
    assert abs(d["value"] - 64 * 64 * 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_plain_run_dumps_what_its_timed_steps_computed(tmp_path):
    """--dump-outputs: r and the matrix values as the timed steps leave them -- the step adds into both, so 2 warm-up and 3
    timed steps hold 5 assemblies -- against the oracle's assembly of the same u.  A plain run measures nothing after its
    timed steps: what --full adds is absent from the line."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from oracle import iga, ref_path as rp
    d = run_bench("--workload", "cfg1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 2 and d["cpu_baseline"] is None and d["roofline"]["phase_ms"] is None
    assert not any(k in d for k in ("per_newton_iteration", "residual_only", "post_time_advance_ms", "other_configs"))
    r, A = np.load(tmp_path / "residual.npy"), np.load(tmp_path / "tangent.npy")
    n_el, p, material = bench.WORKLOADS["cfg1"]
    P = iga.Patch.block(n_el, p)
    D = rp.DomainOracle(P, bench._oracle_material(material))
    r_o, A_o = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(bench.synthetic_u(P), 1.0, r_o, A_o, rp.TANGENT_EXACT)
    assert r.dtype == A.dtype == np.float64 and r.shape == r_o.shape and A.shape == A_o.shape
    assert np.abs(r - 5 * r_o).max() < 1e-12 * np.abs(5 * r_o).max()
    assert np.abs(A - 5 * A_o).max() < 1e-11 * np.abs(5 * A_o).max()


def test_full_run_adds_what_a_plain_run_leaves_out():
    d = run_bench("--workload", "cfg2", "--steps", "2", "--warmup", "1", "--full", MIMI_BENCH_CPU_SAMPLE="4x4x2")
    assert d["steps"] == 2 and d["per_newton_iteration"]["ms"] > d["ms_per_step"] and d["residual_only"]["ms"] > 0.0
    phases = d["roofline"]["phase_ms"]
    assert phases["phase1_integration_kernels"] > 0.0 and phases["phase2_row_gather"] > 0.0
    assert d["roofline"]["binding"] is not None
    assert d["cpu_baseline"]["value"] > 0.0 and abs(d["vs_baseline"] - d["value"] / d["cpu_baseline"]["value"]) < 1e-9 * d["vs_baseline"]


def test_rehearsal_of_one_rank_over_rccl():
    d = run_bench("--rehearse-rccl", "4", "--workload", "cfg2", "--steps", "3", "--warmup", "1")
    assert d["ranks_rehearsed"] == 4 and d["n_gpus"] == 1 and "rehearsal" in d
    assert d["elements_on_this_rank"] == 64 * 64 * 8 // 4
    assert d["ms_per_step"] > 0.0


@pytest.mark.parametrize("launcher", ["own", "torchrun"])
def test_two_ranks_sharing_the_gpu_over_gloo(launcher):
    """the N > 1 code path of bench.py end to end (slabs, two-step assembly, interface exchange, barrier + max-over-ranks
    timing, the owned-rows check against a whole-patch assembly) with both ways of starting the ranks: bench.py's own
    launcher and the driver's `python -m torch.distributed.run`.  Two ranks share the one GPU and exchange over gloo
    (MIMI_BENCH_BACKEND=gloo): the timings mean nothing, the line's contract and the check do."""
    import socket
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["MIMI_BENCH_BACKEND"] = "gloo"
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg2", "--steps", "2", "--warmup", "1"]
    if launcher == "own":
        cmd = [sys.executable] + tail
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + tail
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[:2000]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["name"] == "cfg2"
    assert abs(d["value"] - 64 * 64 * 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    check = d["check"]
    assert check["residual_rel_err"] < 1e-12 and check["tangent_rel_err"] < 1e-12
