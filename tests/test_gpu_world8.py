"""The multi-rank exchanges at world size 8, on hardware: eight processes share cuda:0 through a gloo group (collectives staged
through host memory, as in tests/test_gpu_exchange.py), each writes an .npz, and the parent compares them with the brute-force
oracle (ABI level) or with the same case run in one process (whole runs).  World 8 opens what world 2 never reaches: ranks that own
no rows of the sharded 6x6 reduction, empty query slices, ties held by three ranks, cloud shards of fewer rows than ranks.

One 8-rank group runs at a time and the parent does no GPU work of its own here; in a whole-suite run the parent pytest process
has initialised the GPU in earlier files, so nine processes hold it while a group runs."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORLD = 8
LB, LCH = 512, 2                   # sicp_lm.hip: rows per chunk, chunks per round of the sharded Gram evaluation


def quantised_cloud(n, seed=7):
    """Coordinates on a 0.1 grid (exact distance ties), the first 200 rows copied to n // 2 and 5 n // 6 (three different shards at
    world 8), zeros stored as -0.0 (a bit pattern a SUM would not carry)."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.uniform(-5, 5, (n, 3)), 1)
    X[n // 2:n // 2 + 200] = X[:200]
    X[5 * n // 6:5 * n // 6 + 200] = X[:200]
    X[X == 0.0] = -0.0
    return X


def abi_queries(q, H, X, seed=8):
    """q quantised queries, the last 60 on the triplicated rows under H (winners held by three ranks)."""
    Q = np.round(np.random.default_rng(seed).uniform(-5, 5, (q - 60, 3)), 1)
    return np.vstack((Q, X[:60] @ H[:3, :3].T + H[:3, 3]))


ABI_H = np.array([[0.9950041652780258, -0.09983341664682815, 0.0, 0.3], [0.09983341664682815, 0.9950041652780258, 0.0, 0.1],
                  [0.0, 0.0, 1.0, -0.2], [0.0, 0.0, 0.0, 1.0]])
# 10 000 rows per rank: at Q = 700 a shard is searched by the exact scan (k_knn1_scan: n <= 262 144 and n Q <= 1e9); at
# Q = 196 611 (n Q > 1e9, Q above the filter's default threshold of 196 608 queries) by the grid through the float32 filter
ABI_N = 80_001
ABI_CASES = [dict(name="q700", q=700, max_dist=float("inf"), max_range=0.15, kernel="k_knn1_scan"),
             dict(name="q700_near", q=700, max_dist=0.15, max_range=0.3, kernel="k_knn1_scan"),
             dict(name="q196k", q=196_611, max_dist=float("inf"), max_range=0.15, kernel="k_grid_nn16f")]


def tie_pair(m=20_000):
    """A surface pair whose movable cloud is stored three times over (rows i, i + m, i + 2m: three different ranks at world 8), so
    that EVERY match is an exact tie among three ranks; x coordinates near zero are set to -0.0.  The movable planarity column
    passes the first copy and fails half of the others: a winner other than the lowest index changes the kept set, hence H."""
    sys.path.insert(0, str(ROOT))
    import bench
    Xf, Xm, _ = bench.synthetic_pair(m)
    Xm = np.round(Xm, 2)
    Xm[np.argsort(np.abs(Xm[:, 0]), kind="stable")[:200], 0] = -0.0
    Xm = np.vstack((Xm, Xm, Xm))
    pl = np.ones(3 * m, np.float32)
    pl[m::2] = 0.0
    return Xf, Xm, pl


WORKER = r'''
import os, sys, json, datetime, hashlib, traceback, numpy as np
rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, "%(root)s"); sys.path.insert(0, "%(root)s/tests")
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SIMPLEICP_DEVICE="0")
import torch
torch.set_num_threads(2)                                    # (eight ranks on sixteen CPUs)
import pandas as pd
import bench
from conftest import load_golden, load_cloud
from test_gpu_world8 import quantised_cloud, abi_queries, tie_pair, ABI_H, ABI_N
from simpleicp_amd import PointCloud, SimpleICP, backend, dist, _lib
if world > 1:
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
cases = json.loads(os.environ["SICP_TEST_CASES"])
res = {}

def pair(case):
    kind = case["data"]
    if kind == "synthetic":
        Xf, Xm, _ = bench.synthetic_pair(case["n"])
        return PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]), {}
    if kind == "ties":
        Xf, Xm, pl = tie_pair()
        pm = PointCloud(Xm, columns=["x", "y", "z"]); pm["planarity"] = pl
        return PointCloud(Xf, columns=["x", "y", "z"]), pm, {}
    g, files, kw = load_golden(case["golden"])
    Xf, Xm = load_cloud(files[0]), load_cloud(files[1])
    if kind == "tiny":                                      # a movable cloud of fewer rows than ranks
        Xm = Xm[::len(Xm) // 5][:5]
    if kind == "apart":                                     # nothing within max_overlap_distance
        Xm = Xm + np.array([1000.0, 0.0, 0.0])
    pf = PointCloud(Xf, columns=["x", "y", "z"]); pm = PointCloud(Xm, columns=["x", "y", "z"])
    if "mov_sel_idx" in g.files and kind != "tiny":
        v = np.full(len(pm), np.nan, np.float32)
        v[g["mov_planarity_rows"]] = g["mov_planarity_vals"]
        pm["planarity"] = pd.arrays.SparseArray(v)
        pm.idx_selected = g["mov_sel_idx"][g["mov_sel_idx"] %% 3 != 0]           # a partial selection: shards of the subset
    if kind == "tiny_sel":                                  # ... of fewer rows than ranks, drawn from a larger cloud
        pm.idx_selected = np.arange(5) * (len(Xm) // 5)
    return pf, pm, kw

def run_case(case):
    pf, pm, kw = pair(case)
    icp = SimpleICP(verbose=False); icp.add_point_clouds(pf, pm)
    H, X, rbp, r = icp.run(**{**kw, **case.get("kw", {})})
    info = icp.last_run_info
    ctx = backend.get_context()
    keep = ctx.icp_state(pc2_idx=False, dist=False)[2]
    if world > 1:
        assert info["ranks"] == world and info["exchange"] == "callback", info
        for k in ("partition", "winner_exchange"):
            assert info[k] == case["expect"][k], (case["name"], k, info)
        if case["expect"]["winner_exchange"] == "none":          # (the host-side solve: one exchange per iteration, outside the chain's count)
            assert info["exchanges"] == 0, info
        elif case.get("kw", {}).get("min_change") == 0.0:       # (every iteration ran: the chain did not launch beyond the last)
            assert info["exchanges"] == info["iterations"], info
        else:
            assert info["exchanges"] >= info["iterations"], info
        if "kernel" in case["expect"]:
            assert ctx.last_match_kernel() == case["expect"]["kernel"], (case["name"], ctx.last_match_kernel())
    n = case["name"]
    res[n + "_H"] = H; res[n + "_r"] = r
    # the transformed cloud: every row through a digest of its bytes, and the rows themselves where they are few enough to keep
    res[n + "_Xsha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(X).tobytes()).digest(), np.uint8)
    if len(X) <= 200_000:
        res[n + "_X"] = X
    res[n + "_it"] = np.array(info["iterations"]); res[n + "_Q"] = np.array(len(keep))

def abi_case(case):
    # the ABI level: this rank's index shard of the cloud on a Context of its own, the gloo callback exchange as dist.attach
    # registers it, then the two search entry points that exchange (sicp_knn, sicp_select_in_range)
    X = quantised_cloud(ABI_N)
    Qp = abi_queries(case["q"], ABI_H, X)
    lo, hi = dist.shard_bounds(len(X), rank, world)
    with _lib.Context(0) as ctx:
        ctx.upload(_lib.MOV, X[lo:hi], index_base=lo)
        ctx.upload(_lib.FIX, Qp)
        assert dist.attach(ctx, partition=_lib.PART_CLOUD) == "callback"
        try:
            idx, d2 = ctx.knn(_lib.MOV, Qp, k=1, H=ABI_H, max_dist=case["max_dist"])
            assert ctx.last_match_kernel() == case["kernel"], (case["name"], "knn", ctx.last_match_kernel())
            near = ctx.select_in_range(_lib.FIX, _lib.MOV, None, ABI_H, case["max_range"])
            assert ctx.last_match_kernel() == case["kernel"], (case["name"], "select_in_range", ctx.last_match_kernel())
        finally:
            dist.detach(ctx)
    n = case["name"]
    res[n + "_idx"] = idx[:, 0]; res[n + "_d2"] = d2[:, 0]; res[n + "_near"] = near

for case in cases:
    for k, v in case.get("env", {}).items():
        os.environ[k] = v
    backend.reset_context()
    try:
        if case.get("abi"):
            abi_case(case)
        else:
            run_case(case)
    except AssertionError:
        raise
    except Exception as e:                                  # recorded: a failure case's outcome is compared with one process's
        res[case["name"] + "_err"] = np.array(f"{type(e).__name__}: {e}")
        if not case.get("may_fail"):
            traceback.print_exc()
            raise
    for k in case.get("env", {}):
        del os.environ[k]
if world > 1:
    td.barrier(); td.destroy_process_group()
np.savez(out, **res)
print("RANK_OK", rank, flush=True)
'''


def _launch(tmp_path, cases, world, tag, extra_env=None):
    """`world` worker processes (one group), every communicate() under a deadline; the .npz of every rank."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker8.py"
    script.write_text(WORKER % {"root": str(ROOT)})
    env = {k: v for k, v in os.environ.items() if not k.startswith("SICP_")}
    env["SICP_TEST_CASES"] = json.dumps(cases)
    env.update(extra_env or {})
    outs = [tmp_path / f"{tag}_w{world}_rank{r}.npz" for r in range(world)]
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(port), str(outs[r])], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        logs = [p.communicate(timeout=900)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate(timeout=60)
    assert all(p.returncode == 0 for p in procs) and all("RANK_OK" in o for o in logs), "\n".join(o[-3000:] for o in logs)
    return [np.load(f) for f in outs]


def _release_gpu():
    """The parent does no GPU work in this file: drop the package's process-wide context an earlier test may hold."""
    b = sys.modules.get("simpleicp_amd.backend")
    if b is not None:
        b.reset_context()


def test_world8_abi_exchanges_equal_brute_force(tmp_path):
    """Every rank searches its index shard of a quantised cloud (triplicated rows in three shards, -0.0 coordinates) through
    sicp_knn and sicp_select_in_range with the callback exchange of eight ranks: indices and squared distances bit-identical to the
    fp64 brute force over the WHOLE cloud (k_lexmin_gathered over 8 records, ties held by three ranks).  Q = 700 searches every
    shard by the exact scan, Q = 196 611 by the grid through the float32 filter (k_grid_nn16f) -- every rank asserts the kernel
    after each call; once with a finite max_dist (queries no rank has a candidate for)."""
    sys.path.insert(0, str(ROOT))
    from oracle import orc
    from simpleicp_amd import dist
    X = quantised_cloud(ABI_N)
    owner = lambda row: next(r for r in range(WORLD) if dist.shard_bounds(ABI_N, r, WORLD)[1] > row)
    assert len({owner(row) for row in (0, ABI_N // 2, 5 * ABI_N // 6)}) == 3 and np.signbit(X[X == 0]).all() and (X == 0).any()
    rows = [hi - lo for lo, hi in (dist.shard_bounds(ABI_N, r, WORLD) for r in range(WORLD))]
    assert max(rows) <= 262_144 and max(rows) * 700 <= 1e9 and min(rows) * 196_611 > 1e9      # (knn1_device's route conditions)
    cases = [dict(c, abi=True) for c in ABI_CASES]
    _release_gpu()
    ranks = _launch(tmp_path, cases, WORLD, "abi")
    for c in ABI_CASES:
        Qp = abi_queries(c["q"], ABI_H, X)
        fidx, fd2 = orc.knn(X, Qp, k=1, H=ABI_H, max_dist=c["max_dist"])
        _, rd2 = orc.knn(X, Qp, k=1, H=ABI_H, max_dist=c["max_range"])
        near = np.isfinite(rd2[:, 0])
        # the precondition: winners tied among three ranks were among the cases
        tied = (np.arange(len(Qp)) >= len(Qp) - 60) & (fidx[:, 0] >= 0)
        assert tied.sum() >= 50 and np.isin(fidx[tied, 0], np.arange(200)).all()
        if np.isfinite(c["max_dist"]):
            assert (fidx[:, 0] < 0).any() and (fidx[:, 0] >= 0).any()
        assert near.any() and (~near).any()
        for r, z in enumerate(ranks):
            n = c["name"]
            assert np.array_equal(z[n + "_idx"], fidx[:, 0]), (n, r, np.flatnonzero(z[n + "_idx"] != fidx[:, 0])[:10])
            assert np.array_equal(z[n + "_d2"].view(np.int64), fd2[:, 0].view(np.int64)), (n, r)
            assert np.array_equal(z[n + "_near"].astype(bool), near), (n, r)


def lm_rows(Q, rank, world):
    """launch_lm_eval's share of the rows (sicp_lm.hip): whole rounds of LCH chunks of LB rows, ceil(rounds / world) per rank."""
    nchunks = (Q + LB - 1) // LB
    rounds = (nchunks + LCH - 1) // LCH
    per = (rounds + world - 1) // world
    lo, hi = min(rounds, per * rank) * LCH, min(nchunks, min(rounds, per * (rank + 1)) * LCH)
    return max(0, min(Q, hi * LB) - lo * LB)


def query_slice(Q, rank, world):
    """query_slice (sicp_comm.cpp) and normal_eq_host's slices (sicp_icp.cpp): ceil(Q / world) queries per rank."""
    per = (Q + world - 1) // world
    lo = min(Q, per * rank)
    return min(Q, lo + per) - lo


CLOUD_REC = {"partition": "cloud", "winner_exchange": "records_allgather"}
QSLICES = {"partition": "queries", "winner_exchange": "query_slices"}
KEYS = {"partition": "cloud", "winner_exchange": "key_allreduces"}
RUN_CASES = [
    # cloud shards, records: the overlap pre-pass (k_lexmin_gathered) and the chain (k_lexmin_postmatch)
    dict(name="bunny", data="golden", golden="bunny", expect=CLOUD_REC),
    # shards of a selected subset, the movable planarity column in the merged post-match, Q above the one-workgroup tail
    dict(name="bunny_chain", data="golden", golden="bunny_chain", kw={"correspondences": 30_000}, expect=CLOUD_REC),
    # every match a tie among three ranks: the lexicographic tie-break decides which planarity verdict counts
    dict(name="ties", data="ties", kw={"correspondences": 3000}, expect=CLOUD_REC),
    # three reductions on 8-byte keys over eight ranks (k_xkey_*), the filtered search's slot-bound refresh; a declining callback
    dict(name="q40k", data="synthetic", n=600_000, kw={"correspondences": 40_000, "max_iterations": 6, "min_change": 0.0},
         env={"SICP_GN_SHARD": "0"}, expect=dict(KEYS, kernel="k_grid_nn16")),
    dict(name="q262k", data="synthetic", n=600_000, kw={"correspondences": 262_144, "max_iterations": 6, "min_change": 0.0},
         env={"SICP_GN_SHARD": "0", "SICP_PARTITION": "cloud"}, expect=dict(KEYS, kernel="k_grid_nn16f")),
    dict(name="q40k_declined", data="synthetic", n=600_000, kw={"correspondences": 40_000, "max_iterations": 6, "min_change": 0.0},
         env={"SICP_GN_SHARD": "0", "SICP_XCHG_U64": "0"}, expect=dict(CLOUD_REC, kernel="k_grid_nn16")),
    # query shards: full, short and EMPTY last slices
    dict(name="qs1000", data="golden", golden="bunny", env={"SICP_PARTITION": "queries"}, expect=QSLICES),
    dict(name="qs999", data="golden", golden="bunny", kw={"correspondences": 999}, env={"SICP_PARTITION": "queries"}, expect=QSLICES),
    dict(name="qs41", data="golden", golden="bunny", kw={"correspondences": 41}, env={"SICP_PARTITION": "queries"}, expect=QSLICES),
    # the sharded 6x6 reduction with ranks that own no Gram rows (device solver), and the host solver's slices
    dict(name="gn5000", data="golden", golden="dragon_q5000", env={"SICP_GN_SHARD": "1"}, expect=CLOUD_REC, gn=True),
    dict(name="gn2049", data="synthetic", n=60_000, kw={"correspondences": 2049}, env={"SICP_GN_SHARD": "1"}, expect=CLOUD_REC,
         gn=True),
    dict(name="gn_host", data="golden", golden="bunny", env={"SICP_GN_SHARD": "1", "SICP_SOLVE": "host"},
         expect={"partition": "cloud", "winner_exchange": "none"}, gn=True),
    dict(name="gn_host41", data="golden", golden="bunny", kw={"correspondences": 41}, env={"SICP_GN_SHARD": "1", "SICP_SOLVE": "host"},
         expect={"partition": "cloud", "winner_exchange": "none"}, gn=True),
    # failures: every rank raises what one process raises, and the next run in the same processes is right
    dict(name="fail_planarity", data="golden", golden="bunny", kw={"min_planarity": 1.0}, expect=CLOUD_REC, may_fail=True),
    dict(name="after_planarity", data="golden", golden="bunny", expect=CLOUD_REC),
    dict(name="fail_apart", data="apart", golden="bunny", expect=CLOUD_REC, may_fail=True),
    dict(name="after_apart", data="golden", golden="bunny", expect=CLOUD_REC),
    # cloud shards of fewer rows than ranks: the cloud is replicated (query shards) -- one process's result on every rank
    dict(name="tiny", data="tiny", golden="bunny", kw={"max_overlap_distance": float("inf")}, expect=QSLICES),
    dict(name="tiny_sel", data="tiny_sel", golden="bunny", kw={"max_overlap_distance": float("inf")}, expect=QSLICES),
    dict(name="after_tiny", data="golden", golden="bunny", expect=CLOUD_REC),
]


def test_world8_runs_equal_one_process(tmp_path):
    """SimpleICP.run at world 8 against the same case in one process: H, residuals, the transformed cloud and the iteration count
    bit-identical on every rank (the sharded 6x6 reduction groups its sums by rank: |dH|, |dr| < 1e-9, as at world 2), every
    rank's route asserted (ranks, partition, winner exchange, exchanges, match kernel where pinned).  Failures raise the
    one-process exception on every rank, and the next run is right."""
    _release_gpu()
    # the minimisation as separate launches in BOTH runs: eight processes time-sliced on one GPU cannot keep the one-launch
    # solver's blocks co-resident at its grid barrier (it gives up and reports it; one rank per GPU never meets this)
    lm = {"SICP_LM": "launches"}
    one = _launch(tmp_path, RUN_CASES, 1, "run", lm)[0]
    eight = _launch(tmp_path, RUN_CASES, WORLD, "run", lm)
    # the preconditions the cases are there for, restated from launch_lm_eval / query_slice
    Q = lambda n: int(one[n + "_Q"])
    assert Q("gn5000") == 5000 and [lm_rows(5000, r, WORLD) > 0 for r in range(WORLD)] == [True] * 5 + [False] * 3   # ranks 5-7 own no chunks
    assert Q("gn2049") == 2049 and [lm_rows(2049, r, WORLD) > 0 for r in range(WORLD)] == [True] * 3 + [False] * 5   # ranks 3-7 own none
    assert sum(lm_rows(5000, r, WORLD) for r in range(WORLD)) == 5000 and sum(lm_rows(2049, r, WORLD) for r in range(WORLD)) == 2049
    assert Q("qs41") == 41 and query_slice(41, 7, WORLD) == 0 and query_slice(41, 6, WORLD) == 5       # rank 7's slice is empty
    assert Q("qs999") == 999 and query_slice(999, 7, WORLD) == 124 and Q("qs1000") == 1000 and query_slice(1000, 7, WORLD) == 125
    assert Q("gn_host") > 0 and all(query_slice(Q("gn_host"), r, WORLD) > 0 for r in range(WORLD))
    assert Q("gn_host41") == 41 and query_slice(41, 7, WORLD) == 0                                      # normal_eq_host: rank 7 sums nothing
    assert Q("bunny_chain") > 2048 and Q("ties") == 3000 and Q("q262k") == 262_144
    # the failure cases did fail in one process, the rest did not
    for c in RUN_CASES:
        assert (c["name"] + "_err" in one) == c["name"].startswith("fail_"), (c["name"], str(one.get(c["name"] + "_err")))
    assert "Too few correspondences" in str(one["fail_planarity_err"]) and "overlap" in str(one["fail_apart_err"])
    for r, z in enumerate(eight):
        for c in RUN_CASES:
            n = c["name"]
            if n.startswith("fail_"):
                assert n + "_H" not in z and str(z[n + "_err"]) == str(one[n + "_err"]), (n, r, str(z.get(n + "_err")))
                continue
            assert n + "_err" not in z, (n, r, str(z[n + "_err"]))
            assert int(z[n + "_it"]) == int(one[n + "_it"]) and int(z[n + "_Q"]) == Q(n), (n, r)
            if c.get("gn"):
                assert np.abs(z[n + "_H"] - one[n + "_H"]).max() < 1e-9, (n, r, np.abs(z[n + "_H"] - one[n + "_H"]).max())
                assert np.abs(z[n + "_r"] - one[n + "_r"]).max() < 1e-9, (n, r)
                # every row of the transformed cloud, to what the bar on H implies: X = R p + t moves by at most
                # |dR| (|p_x| + |p_y| + |p_z|) + |dt| <= 1e-9 (sqrt(3) |p| + 1), |p| = |X - t| (R preserves lengths), plus the
                # rounding of the two products (a few ulp of that scale)
                X1 = one[n + "_X"]
                scale = np.sqrt(3) * np.linalg.norm(X1 - one[n + "_H"][:3, 3], axis=1).max() + 1.0
                tol = 1e-9 * scale + 8 * np.finfo(float).eps * (scale + np.abs(one[n + "_H"][:3, 3]).max())
                assert np.abs(z[n + "_X"] - X1).max() <= tol, (n, r, np.abs(z[n + "_X"] - X1).max(), tol)
            else:
                assert np.array_equal(z[n + "_H"], one[n + "_H"]), (n, r, np.abs(z[n + "_H"] - one[n + "_H"]).max())
                assert np.array_equal(z[n + "_r"], one[n + "_r"]), (n, r)
                assert np.array_equal(z[n + "_Xsha"], one[n + "_Xsha"]), (n, r)                # every row, bit for bit


def test_bench_eight_ranks_self_launched():
    """`python bench.py --gpus 8` in share mode (every rank on cuda:0 over gloo): ONE JSON line, eight ranks in the exchange, the
    parity legs green."""
    _release_gpu()
    env = dict(os.environ, SICP_BENCH_SHARE_GPU="1")
    args = [str(ROOT / "bench.py"), "--full", "--gpus", "8", "--steps", "3", "--warmup", "1", "--repeats", "1", "--points", "1000000",
            "--partition", "cloud", "--no-cpu-baseline", "--no-end-to-end", "--no-bruteforce-leg", "--throughput-q", "40000",
            "--throughput-repeats", "1"]
    r = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["comm"]["nranks"] == 8, d["comm"]
    assert d["parity"]["ok"] is True, d["parity"]
    assert d["throughput_point"]["parity"]["ok"] is True, d["throughput_point"]
