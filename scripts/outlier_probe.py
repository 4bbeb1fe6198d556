"""Measurements of the outlier filters (records under profiles/outlier/).

    python scripts/outlier_probe.py cost [--runs R] [--out FILE]   what both filters cost, next to estimate_normals on the same rows
    python scripts/outlier_probe.py icp  [--runs R] [--out FILE]   what the statistical filter buys on a pair with planted strays

cost: on bench.py's 10 M-point uniform cloud and its 1.25 M-point terrestrial stand-in, every point a candidate, the cloud already
  in the slot: wall time of Context.outlier_statistical (k = 20, verdicts into device memory), of Context.estimate_normals_into for
  the same rows and the same k -- the same sweep followed by a heavier epilogue: the yardstick --, and of Context.outlier_radius
  with radius = twice the mean nearest-neighbour spacing (measured with sicp_knn on a sample) and min_points = 5, with the
  candidates the walk read per query (the library's work tallies) and its share of HBM peak on algorithmic bytes (24 B read + 5 B
  written per candidate).  Each after a warm-up, between device synchronisations, median of R.  No torch baseline is timed: the
  same computation in torch needs the n x n distances (in memory, or 10^14 of them recomputed chunk by chunk at 10 M points).
  For kernel times run it under `rocprofv3 --kernel-trace --stats` (a run of its own: --runs 3).
icp: run_tensors on the terrestrial pair with 1 % strays planted in the fixed cloud, Q = 10 000, without and with
  outlier_neighbors = 20: iterations and the distance of H from the pair's ground truth.
One JSON line per record; --out appends them to a file.

How the records under profiles/outlier/ are made -- every GPU step under a time limit of its own, the steps chained so that a
failing one ends the sequence, the profiler in a run of its own:

    timeout -k 10 300 python scripts/outlier_probe.py cost --runs 7 --out cost.jsonl && \
    timeout -k 10 240 python scripts/outlier_probe.py icp --out icp.jsonl && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d trace -o cost -- \
        python scripts/outlier_probe.py cost --runs 3"""
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
from simpleicp_amd import _lib, backend

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["cost", "icp"])
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
HBM_PEAK_GBPS = 8000.0


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


def cost():
    clouds = [("uniform_10M", bench.synthetic_pair(10_000_000)[0]), ("terrestrial_1.25M", bench.terrestrial_pair(1_250_000)[0])]
    ctx = backend.get_context()
    k = 20
    for name, Xh in clouds:
        n = len(Xh)
        ctx.upload(_lib.FIX, np.ascontiguousarray(Xh))
        sample = Xh[:: max(n // 20_000, 1)]
        spacing = float(np.sqrt(ctx.knn(_lib.FIX, sample, k=2)[1][:, 1]).mean())
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        rec = {"mode": "cost", "cloud": name, "n": n, "k": k, "mean_nn_spacing": round(spacing, 5)}
        st = ctx.outlier_statistical(_lib.FIX, k, 2.0, keep_ptr=keep.data_ptr())
        rec["statistical"] = dict(st.as_dict(), **timed(lambda: ctx.outlier_statistical(_lib.FIX, k, 2.0, keep_ptr=keep.data_ptr()), args.runs))
        sel = torch.arange(n, dtype=torch.int64, device=DEV)
        nv = torch.empty((n, 3), dtype=torch.float32, device=DEV)
        pl = torch.empty(n, dtype=torch.float32, device=DEV)
        rec["estimate_normals_same_rows"] = timed(lambda: ctx.estimate_normals_into(_lib.FIX, sel.data_ptr(), n, k, nv.data_ptr(), pl.data_ptr()),
                                                  args.runs)
        r, mp = 2.0 * spacing, 5
        cnt = torch.empty(n, dtype=torch.int32, device=DEV)
        rec["radius"] = {"radius": round(r, 5), "min_points": mp, "box_cells": ctx.outlier_radius_cells(_lib.FIX, r)}
        rec["radius"]["kept"] = ctx.outlier_radius(_lib.FIX, r, mp, keep_ptr=keep.data_ptr(), count_ptr=cnt.data_ptr())
        rec["radius"].update(timed(lambda: ctx.outlier_radius(_lib.FIX, r, mp, keep_ptr=keep.data_ptr(), count_ptr=cnt.data_ptr()), args.runs))
        ctx.timing_enable(True, count_work=True)                                      # the searches also tally their candidates and rows
        before = ctx.match_work()
        ctx.outlier_radius(_lib.FIX, r, mp, keep_ptr=keep.data_ptr())
        after = ctx.match_work()
        ctx.timing_enable(False)
        rec["radius"]["candidates_read_per_query"] = round((after["candidates"] - before["candidates"]) / n, 2)
        rec["radius"]["rows_per_query"] = round((after["rows"] - before["rows"]) / n, 2)
        rec["radius"]["algorithmic_bytes"] = 29 * n
        gbps = 29 * n / rec["radius"]["median_us"] / 1e3
        rec["radius"]["GBps_of_algorithmic_bytes"] = round(gbps, 1)
        rec["radius"]["share_of_hbm_peak"] = round(gbps / HBM_PEAK_GBPS, 4)
        emit(rec)
        del keep, sel, nv, pl, cnt
        torch.cuda.empty_cache()


def h_distance(H, H_true):
    """(rotation angle in degrees, translation distance) between H and the ground truth"""
    D = np.linalg.inv(H_true) @ H
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return round(float(ang), 5), round(float(np.linalg.norm(D[:3, 3])), 5)


def icp():
    Xf, Xm, H_true = bench.terrestrial_pair(1_250_000)
    rng = np.random.default_rng(7)
    at = rng.choice(len(Xf), len(Xf) // 100, replace=False)          # 1 % strays: returns displaced along their ray by up to 2 m
    Xf = Xf.copy()
    Xf[at] *= (1.0 + rng.uniform(-0.5, 0.5, len(at)) * 2.0 / np.maximum(np.linalg.norm(Xf[at], axis=1), 2.0))[:, None]
    Tf, Tm = (torch.tensor(a, dtype=torch.float64, device=DEV) for a in (Xf, Xm))
    for name, extra in (("as_today", {}), ("outlier_neighbors_20", {"outlier_neighbors": 20})):
        t0 = time.perf_counter()
        res = simpleicp_amd.run_tensors(Tf, Tm, correspondences=10_000, **extra)
        ang, tr = h_distance(res.H, H_true)
        emit({"mode": "icp", "way": name, "n_fixed": len(Tf), "strays": len(at), "iterations": res.iterations, "n_kept": res.n_kept,
              "H_rotation_error_deg": ang, "H_translation_error": tr, "outlier": res.outlier,
              "wall_s": round(time.perf_counter() - t0, 3)})


if not torch.cuda.is_available():
    sys.exit("outlier_probe.py needs a GPU")
{"cost": cost, "icp": icp}[args.mode]()
