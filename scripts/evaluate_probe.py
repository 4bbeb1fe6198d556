"""Measurements of the evaluation (records under profiles/evaluate/).

    python scripts/evaluate_probe.py [--points N] [--runs R] [--distance D] [--out FILE]

On bench.py's C4 pair (10 M vs 10 M, the pair's known rigid transform as the converged H, max_distance = 1): wall time of
Context.evaluate over ALL fixed points next to Context.select_in_range_into with the same arguments (its verdicts left in device
memory) and Context.select_in_range (its 10 MB mask downloaded), in the same process, each after a warm-up, between device
synchronisations, median / min / max of R.  On a checkout that has no evaluation (the parent commit) the select_in_range records
alone are written: they are the yardstick.  The record's figures (fitness, RMSE) and the count of the mask are written too, and
compared.  One JSON line per record; --out appends them to a file.

For the kernel times run it under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host, wall times come
from the plain run).  How the records under profiles/evaluate/ are made -- every GPU step under a time limit of its own, the
steps chained so that a failing one ends the sequence:

    timeout -k 10 300 python scripts/evaluate_probe.py --runs 9 --out wall.jsonl && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d trace -o eval -- \
        python scripts/evaluate_probe.py --runs 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from simpleicp_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=10_000_000)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--distance", type=float, default=1.0)
ap.add_argument("--out", default="")
args = ap.parse_args()


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
    return {"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t)), "runs": runs}


Xf, Xm, H_true = bench.synthetic_pair(args.points)
H = np.asarray(H_true, dtype=np.float64).reshape(4, 4)
d = args.distance
has_eval = hasattr(_lib.Context, "evaluate")
base = {"points": args.points, "max_distance": d, "csrc": bench.csrc_hash(), "has_evaluate": has_eval}

with _lib.Context(0) as ctx:
    ctx.upload(_lib.FIX, Xf)
    ctx.upload(_lib.MOV, Xm)
    mask_dev = torch.empty(len(Xf), dtype=torch.uint8, device="cuda:0")
    emit(dict(base, call="select_in_range_into", **timed(lambda: ctx.select_in_range_into(_lib.FIX, _lib.MOV, H, d, mask_dev.data_ptr()),
                                                         args.runs), in_range=int(mask_dev.sum().item())))
    emit(dict(base, call="select_in_range", **timed(lambda: ctx.select_in_range(_lib.FIX, _lib.MOV, None, H, d), args.runs)))
    if has_eval:
        from simpleicp_amd import Evaluation
        emit(dict(base, call="evaluate", **timed(lambda: ctx.evaluate(_lib.FIX, _lib.MOV, H, d), args.runs)))
        ev = Evaluation.from_record(ctx.evaluate(_lib.FIX, _lib.MOV, H, d))
        emit(dict(base, call="evaluate_record", n_queries=ev.n_queries, n_inliers=ev.n_inliers, fitness=ev.fitness,
                  inlier_rmse=ev.inlier_rmse, agrees_with_mask=bool(ev.n_inliers == int(mask_dev.sum().item())),
                  bytes_reduced=40 * ev.n_queries))
