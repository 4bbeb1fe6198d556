"""Measurements of the voxel selection (records under profiles/voxel/).

    python scripts/voxel_probe.py cost [--runs R] [--out FILE]     what the selection costs, against torch.unique on the same GPU
    python scripts/voxel_probe.py icp  [--runs R] [--out FILE]     what thinning buys on the non-uniform (terrestrial) pair

cost: on bench.py's 10 M-point uniform cloud and its 1.25 M-point terrestrial stand-in, three cell sizes each (from "almost every
  point its own voxel" to "a few thousand voxels"): wall time of simpleicp_amd.voxel_keep (ingest + both passes + the count; the call
  returns complete), of Context.voxel_select alone on the cloud already in the slot, and of what a user would otherwise write in
  torch in the same process -- a packed int64 key, torch.unique(return_inverse=True), scatter_reduce(amin) --, each after a warm-up,
  between device synchronisations, median of R.  The two keep masks are compared.  For kernel times run it under
  `rocprofv3 --kernel-trace --stats` (a run of its own: --runs 3).
icp: run_tensors on the terrestrial pair at Q = 10 000 as it is, with voxel_size on the fixed side, and with the movable cloud
  thinned by voxel_keep as well: iterations and the distance of H from the pair's ground truth of a whole run, and the
  microseconds per iteration of a fixed 30-iteration sicp_icp_run (min_change = 0) on the same preparation, with the library's own
  per-kernel timing of the match.
One JSON line per record; --out appends them to a file.

How the records under profiles/voxel/ are made -- every GPU step under a time limit of its own, the steps chained so that a failing
one ends the sequence, the profiler in a run of its own (tracing slows the host: wall times come from the plain runs):

    timeout -k 10 300 python scripts/voxel_probe.py cost --runs 9 --out cost.jsonl && \
    timeout -k 10 240 python scripts/voxel_probe.py icp --runs 7 --out icp.jsonl && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d trace -o cost -- \
        python scripts/voxel_probe.py cost --runs 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import simpleicp_amd
from simpleicp_amd import _lib, backend, batch, tensors

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["cost", "icp"])
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, runs):
    """median / min / max wall time in microseconds of fn(), device idle before and after each call"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def torch_keep(X, c):
    """the user's own version: packed int64 key -> unique -> lowest index per key.  (It takes no origin: cost() measures with
    the default origin of zeros, where floor(X / c) is the contract's floor((X - 0) / c) bit for bit.)"""
    v = torch.floor(X / c)
    v = (v - v.amin(dim=0)).to(torch.int64)
    key = (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]
    _, inv = torch.unique(key, return_inverse=True)
    idx = torch.arange(len(X), device=X.device)
    first = torch.full((int(inv.max()) + 1,), len(X), dtype=torch.int64, device=X.device).scatter_reduce(0, inv, idx, "amin")
    keep = torch.zeros(len(X), dtype=torch.bool, device=X.device)
    keep[first] = True
    return keep


def cost():
    clouds = [("uniform_10M", bench.synthetic_pair(10_000_000)[0], (0.05, 0.5, 40.0)),
              ("terrestrial_1.25M", bench.terrestrial_pair(1_250_000)[0], (0.005, 0.1, 4.0))]
    ctx = backend.get_context()
    for name, Xh, cells in clouds:
        X = torch.tensor(Xh, dtype=torch.float64, device=DEV)
        n = len(X)
        for c in cells:
            keep = simpleicp_amd.voxel_keep(X, c)
            ref = torch_keep(X, c)
            rec = {"mode": "cost", "cloud": name, "n": n, "cell": c, "kept": int(keep.sum()), "equals_torch": bool(torch.equal(keep, ref))}
            rec["voxel_keep"] = timed(lambda: simpleicp_amd.voxel_keep(X, c), args.runs)
            out = torch.empty(n, dtype=torch.uint8, device=DEV)
            rec["voxel_select_resident"] = timed(lambda: ctx.voxel_select(_lib.FIX, c, keep_ptr=out.data_ptr()), args.runs)
            rec["torch_unique"] = timed(lambda: torch_keep(X, c), args.runs)
            # algorithmic bytes of the selection itself: 24 read + 1 written per candidate
            rec["algorithmic_bytes"] = 25 * n
            rec["resident_GBps_of_algorithmic_bytes"] = round(25 * n / rec["voxel_select_resident"]["median_us"] / 1e3, 1)
            emit(rec)
            del keep, ref, out
        del X
        torch.cuda.empty_cache()


def h_distance(H, H_true):
    """(rotation angle in degrees, translation distance) between H and the ground truth"""
    D = np.linalg.inv(H_true) @ H
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return round(float(ang), 5), round(float(np.linalg.norm(D[:3, 3])), 5)


def icp():
    Xf, Xm, H_true = bench.terrestrial_pair(1_250_000)
    Tf, Tm = (torch.tensor(a, dtype=torch.float64, device=DEV) for a in (Xf, Xm))
    cell = 0.25
    Tm_thin = Tm[simpleicp_amd.voxel_keep(Tm, cell)].contiguous()
    ways = [("as_today", Tm, {}), ("voxel_fixed", Tm, {"voxel_size": cell}), ("voxel_fixed_and_movable_thinned", Tm_thin, {"voxel_size": cell})]
    ctx = backend.get_context()
    z = np.zeros(6)
    for name, mov, extra in ways:
        res = simpleicp_amd.run_tensors(Tf, mov, correspondences=10_000, **extra)
        ang, tr = h_distance(res.H, H_true)
        rec = {"mode": "icp", "way": name, "n_fixed": len(Tf), "n_movable": len(mov), "cell": cell if extra else None,
               "iterations": res.iterations, "n_kept": res.n_kept, "H_rotation_error_deg": ang, "H_translation_error": tr}
        kw, extras = batch.merged_keywords("voxel_probe", dict(batch._EXTRA_DEFAULTS, **extra), {"correspondences": 10_000})
        _, _, scratch = tensors.prepare(ctx, Tf, mov, kw, extras, lambda *a: None)
        rec["Q"] = ctx._Q
        x = np.array(ctx.icp_run(z, z, z, 0.3, 1.0, max_iterations=12, min_change=0.0)[-1].x[:])      # settle (untimed)
        per = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            r = ctx.icp_run(x, z, z, 0.3, 1.0, max_iterations=30, min_change=0.0)
            per.append((time.perf_counter() - t0) / len(r) * 1e6)
        rec["us_per_iteration"] = {"median": round(float(np.median(per)), 2), "min": round(min(per), 2), "max": round(max(per), 2)}
        ctx.timing_enable(True)
        ctx.timing_reset()
        ctx.icp_run(x, z, z, 0.3, 1.0, max_iterations=30, min_change=0.0)
        tm = ctx.timing()
        ctx.timing_enable(False)
        rec["match_us_per_launch_event_timed"] = round(tm["match"]["ms"] * 1e3 / max(tm["match"]["launches"], 1), 2)
        rec["match_kernel"] = ctx.last_match_kernel()
        emit(rec)
        del scratch


if not torch.cuda.is_available():
    sys.exit("voxel_probe.py needs a GPU")
{"cost": cost, "icp": icp}[args.mode]()
