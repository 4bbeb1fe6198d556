"""Times the batch against loops of lone runs: B in {1, 8, 64, 256} pairs of a 100 k vs 100 k synthetic pair (seeded, made
here) at Q = 1 000.  Prints one JSON line per B:
  run_batch wall time vs a loop of SimpleICP.run (fresh PointClouds each),
  sicp_icp_run_batch vs a loop of sicp_icp_run on the same prepared member contexts (both re-prepared identically),
  where run_batch's time goes (host preparation / batched loops / results: simpleicp_amd.batch.last_run_info),
  and the device memory the member contexts hold (free memory before and after the pool is made and prepared).
Everything is warm: the pool holds max(B) prepared contexts and every path has run at max(B) once before the first timing.
The per-iteration kernel time of the batch comes from a run of its own under rocprofv3 --kernel-trace --stats
(`--only-batch B` runs just the batched call, for that trace).

    python scripts/batch_sweep.py [--sizes 1,8,64,256] [--n 100000] [--q 1000] [--only-batch B]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from simpleicp_amd import PointCloud, SimpleICP, _lib, backend, run_batch  # noqa: E402
from simpleicp_amd import batch as batch_mod  # noqa: E402


def synthetic_pair(n, seed):
    """Two samplings of one analytic surface (10 points per m^2), the movable one under a small rigid motion."""
    L = np.sqrt(n / 10.0)

    def sample(s):
        rng = np.random.default_rng(s)
        x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
        z = 20 * np.sin(2 * np.pi * x / 200) * np.cos(2 * np.pi * y / 300) \
            + 5 * np.sin(2 * np.pi * x / 37 + 1) * np.sin(2 * np.pi * y / 53) + rng.normal(0, 0.02, n)
        return np.column_stack((x, y, z))
    Xf, Xm = sample(2 * seed), sample(2 * seed + 1)
    c0 = Xf.mean(axis=0)
    a = np.deg2rad(0.5)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return Xf - c0, (Xm - c0) @ R.T + np.array([0.3, -0.2, 0.1])


def prepare(ctx, Xf, Xm, q):
    ctx.upload(_lib.FIX, Xf)
    ctx.upload(_lib.MOV, Xm)
    sel = np.unique(np.round(np.linspace(0, len(Xf) - 1, q)).astype(np.int64))
    nv, pl = ctx.estimate_normals(_lib.FIX, sel, 10)
    ctx.icp_setup(sel, nv, pl)


KW = dict(x=np.zeros(6), obs=np.zeros(6), obs_weight=np.zeros(6), min_planarity=0.3, distance_weight=1.0, max_iterations=100,
          min_change=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--q", type=int, default=1000)
    ap.add_argument("--only-batch", type=int, default=0)
    a = ap.parse_args()
    sizes = [a.only_batch] if a.only_batch else [int(s) for s in a.sizes.split(",")]
    Bmax = max(sizes)
    pairs = [synthetic_pair(a.n, s) for s in range(Bmax)]
    probe = _lib.Context(0)
    free0, _ = probe.device_memory()
    ctxs = [_lib.Context(0) for _ in range(Bmax)]
    for c in ctxs:
        c.make_lean()
    # warm-up at max(B): kernels loaded, pools and workspaces sized, every path run once
    for (Xf, Xm), c in zip(pairs, ctxs):
        prepare(c, Xf, Xm, a.q)
    free1, _ = probe.device_memory()
    ctxs[0].icp_run_batch([(c, KW) for c in ctxs])
    run_batch(pairs, correspondences=a.q)
    for Xf, Xm in pairs[:2]:
        icp = SimpleICP(verbose=False)
        icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]))
        icp.run(correspondences=a.q)
    print(json.dumps(dict(members=Bmax, n=a.n, Q=a.q, device_bytes_per_prepared_member=(free0 - free1) / Bmax)), flush=True)
    for B in sizes:
        for (Xf, Xm), c in zip(pairs[:B], ctxs[:B]):
            prepare(c, Xf, Xm, a.q)
        t0 = time.perf_counter()
        runs, fb = ctxs[0].icp_run_batch([(c, KW) for c in ctxs[:B]])
        t_batch = time.perf_counter() - t0
        iters = [len(r.results) for r in runs]
        if a.only_batch:
            print(json.dumps(dict(B=B, c_batch_ms=t_batch * 1e3, iterations_max=max(iters), fallback=fb)), flush=True)
            continue
        for (Xf, Xm), c in zip(pairs[:B], ctxs[:B]):
            prepare(c, Xf, Xm, a.q)
        t0 = time.perf_counter()
        for c in ctxs[:B]:
            c.icp_run(**KW)
        t_loop = time.perf_counter() - t0
        t0 = time.perf_counter()
        run_batch(pairs[:B], correspondences=a.q)
        t_rb = time.perf_counter() - t0
        phases = {k: v * 1e3 for k, v in batch_mod.last_run_info.items() if k.endswith("_s")}
        t0 = time.perf_counter()
        for Xf, Xm in pairs[:B]:
            icp = SimpleICP(verbose=False)
            icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]))
            icp.run(correspondences=a.q)
        t_run = time.perf_counter() - t0
        print(json.dumps(dict(B=B, n=a.n, Q=a.q, iterations_max=max(iters), iterations_sum=sum(iters), fallback=fb,
                              c_batch_ms=t_batch * 1e3, c_loop_ms=t_loop * 1e3, run_batch_ms=t_rb * 1e3, run_loop_ms=t_run * 1e3,
                              c_speedup=t_loop / t_batch, run_speedup=t_run / t_rb,
                              run_batch_phases_ms={k[:-2]: v for k, v in phases.items()})), flush=True)
    backend.reset_batch_contexts()
    probe.close()
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
