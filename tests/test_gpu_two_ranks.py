"""Two ranks sharing cuda:0 (gloo carries the collectives; RCCL refuses two ranks on one
device): the sharded pipeline end to end on real kernels, checked against the oracle."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_one_gpu():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533",
                        os.path.join(ROOT, "scripts", "two_rank_one_gpu.py")], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("match_ok=True ransac_ok=True pipelined_ok=True") == 2     # incl. two registrations in flight per rank


def test_one_rank_rccl_rehearsal_of_every_collective():
    """PCREG_FORCE_COLLECTIVES=1 sends a one-rank job through the whole N > 1 protocol on RCCL (backend "nccl"):
    both all_gathers, the MAX / SUM all_reduces of the matcher and the three of the hypothesis-split RANSAC.
    The registration it finds must be the one the plain single-GPU step finds."""
    import json
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras", "--model-points", "200000", "--surface-points", "20000",
              "--in-flight", "1"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PCREG_FORCE_COLLECTIVES="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29541", os.path.join(ROOT, "bench.py")] + common,
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    forced = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    env2 = {k: v for k, v in os.environ.items() if k != "PCREG_FORCE_COLLECTIVES"}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common, capture_output=True, text=True, env=env2, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    plain = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert forced["ransac"] == plain["ransac"] and not plain["ransac"]["failed"] and plain["ransac"]["n_pairs"] > 1000
    # the same protocol with TWO registrations in flight (two HIP streams issuing their RCCL collectives in host program order)
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                         "--master-addr", "127.0.0.1", "--master-port", "29543", os.path.join(ROOT, "bench.py")] + common[:-2] + ["--in-flight", "2", "--steps", "4"],
                        capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    piped = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    assert piped["in_flight"] == 2 and piped["ransac"] == plain["ransac"]


def test_bench_n2_control_flow_on_one_gpu():
    """bench.py --gpus 2 end to end with both ranks on cuda:0 and gloo carrying the collectives (RCCL refuses two ranks on
    one device): the strong-scaling headline on the FIXED model, cfg 3's 2 M model, the weak-scaling run and cfg 5's batch
    dealt over two ranks all run and agree with the one-rank line where they must (same registration found)."""
    import json
    small = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--model-points", "200000", "--surface-points", "20000", "--crops", "4"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PCREG_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--in-flight", "1"] + small,
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    two = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["model_points_total"] == 200000
    # the dominant kernel is timed on a SMALL shard too (100 k rows: round 2's Q * M >= 2^33 guard would have blanked it,
    # exactly at the 125 k-row shards of the 8-GPU run), once per step, and the roofline is priced from that duration
    assert two["knn_kernel"]["launches_timed"] == 2 and 0.0 < two["knn_kernel"]["ms"] < two["knn_kernel"]["search_call_ms"]
    assert "100000 rows per GPU" in two["config"]["workload"]
    for k in ("cfg3_model_2M", "weak_1M_per_gpu", "cfg5_batch"):
        assert k in two, k
    assert two["cfg3_model_2M"]["scaling"] == "strong" and two["weak_1M_per_gpu"]["scaling"] == "weak"
    assert two["cfg5_batch"]["failed"] == 0 and two["cfg5_batch"]["n_gpus"] == 2
    env1 = {k: v for k, v in os.environ.items() if k not in ("PCREG_BENCH_SHARE_GPU", "PCREG_FORCE_COLLECTIVES")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-extras"] + small, capture_output=True, text=True,
                       env=env1, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    one = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert two["ransac"] == one["ransac"] and not one["ransac"]["failed"]          # the sharded run finds the single-GPU registration
    # the DEFAULT form of the line (two registrations in flight per rank), two ranks: same registration, headline fields in place
    d = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29549", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-extras", "--steps", "4"] + small[2:],
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert d.returncode == 0, d.stdout[-2000:] + d.stderr[-3000:]
    dd = json.loads([l for l in d.stdout.splitlines() if l.startswith("{")][-1])
    assert dd["in_flight"] == 2 and dd["n_gpus"] == 2 and dd["ransac"] == one["ransac"] and dd["knn_kernel"]["launches_timed"] == 4
