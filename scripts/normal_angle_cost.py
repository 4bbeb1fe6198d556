"""What the rejection by the angle between normals costs per iteration, on bench.py's synthetic pair.

    python scripts/normal_angle_cost.py [n_points] [Q ...] [--angle DEG] [--runs R] [--out FILE]

Per Q, wall time of whole sicp_icp_run calls (min_change = 0: a fixed number of iterations), warm (one untimed run first):
  off       the setting off: R runs of IT iterations from the same start, per-iteration time of each (their spread is the
            run-to-run spread a comparison with the parent commit has to stay within -- run this script on both);
  on cold   the setting on, the movable slot's cache emptied before the run (an upload): every iteration's misses are estimated;
  on settled the same run again: every normal is cached, the miss list is empty;
  first     ONE iteration from the start estimate, off and then on with an empty cache: every planar correspondence misses, all
            of their normals are estimated in that iteration (the case the four-queries-per-wave sweep over the list is for).
Prints one JSON line per Q; --out appends them to a file.  On the parent commit only the `off` leg runs."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
from simpleicp_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("points", nargs="?", type=float, default=10_000_000)
ap.add_argument("Q", nargs="*", type=float, default=[1000, 100_000])
ap.add_argument("--angle", type=float, default=30.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--iterations", type=int, default=30)
ap.add_argument("--out", default="")
ap.add_argument("--off-only", action="store_true", help="the `off` leg alone (what the parent commit can run), tagged with --tag")
ap.add_argument("--tag", default="")
args = ap.parse_args()

N, IT = int(args.points), args.iterations
Xf, Xm, _ = bench.synthetic_pair(N)
c = _lib.Context(0)
c.upload(_lib.FIX, Xf)
c.upload(_lib.MOV, Xm)
z = np.zeros(6)
has_feature = hasattr(c, "normal_angle_set") and not args.off_only
cos_max = math.cos(math.radians(args.angle))


def timed_run(x):
    t = time.perf_counter()
    r = c.icp_run(x, z, z, 0.3, 1.0, max_iterations=IT, min_change=0.0)
    return (time.perf_counter() - t) / len(r) * 1e6, r


for Q in (int(q) for q in args.Q):
    sel = np.unique(np.round(np.linspace(0, N - 1, Q)).astype(np.int64))
    nv, pl = c.estimate_normals(_lib.FIX, sel, 10)
    c.icp_setup(sel, nv, pl)
    x = np.array(c.icp_run(z, z, z, 0.3, 1.0, max_iterations=12, min_change=0.0)[-1].x[:])     # settle the estimate (untimed)
    timed_run(x)
    off = [timed_run(x)[0] for _ in range(args.runs)]
    rec = {"n": N, "Q": len(sel), "iterations": IT, "off_us_per_iteration": [round(v, 2) for v in off],
           "off_spread_us": round(max(off) - min(off), 2), "off_median_us": round(float(np.median(off)), 2)}
    if args.tag:
        rec["tag"] = args.tag
    if has_feature:
        c.upload(_lib.MOV, Xm)                       # (empties the cache; the grid is rebuilt by the warm-up below)
        c.icp_setup(sel, nv, pl)
        timed_run(x)                                 # warm: grid, buffers -- feature still off
        c.upload(_lib.MOV, Xm)
        c.icp_setup(sel, nv, pl)
        c.icp_run(x, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0)      # the grid again, outside the timed run
        c.normal_angle_set(cos_max, 10)
        cold, r = timed_run(x)
        info = c.normal_angle_info()
        settled = [timed_run(x)[0] for _ in range(args.runs)]
        info2 = c.normal_angle_info()
        c.normal_angle_set(None)
        # one iteration in which everything misses: off first (same state: grid built, an earlier match to bound the search), then on
        c.upload(_lib.MOV, Xm)
        c.icp_setup(sel, nv, pl)
        c.icp_run(z, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0)
        t = time.perf_counter(); c.icp_run(z, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0); first_off = (time.perf_counter() - t) * 1e6
        c.normal_angle_set(cos_max, 10)
        c.icp_run(z, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0)      # (allocates the cache and the lists: untimed)
        c.upload(_lib.MOV, Xm)                       # ... and empties the cache again
        c.icp_setup(sel, nv, pl)
        c.normal_angle_set(None)
        c.icp_run(z, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0)      # the grid and a previous match, feature off
        c.normal_angle_set(cos_max, 10)
        t = time.perf_counter(); c.icp_run(z, z, z, 0.3, 1.0, max_iterations=1, min_change=0.0); first_on = (time.perf_counter() - t) * 1e6
        first_info = c.normal_angle_info()
        c.normal_angle_set(None)
        rec.update(first_iteration_off_us=round(first_off, 1), first_iteration_on_all_miss_us=round(first_on, 1),
                   first_iteration_normals_estimated=first_info["normals_estimated"],
                   first_iteration_dropped=first_info["normal_angle_dropped"])
        rec.update(angle_deg=args.angle, on_cold_us_per_iteration=round(cold, 2),
                   on_settled_us_per_iteration=[round(v, 2) for v in settled],
                   added_cold_us=round(cold - float(np.median(off)), 2),
                   added_settled_us=round(float(np.median(settled)) - float(np.median(off)), 2),
                   normals_estimated_per_iteration=round(info["normals_estimated"] / IT, 1),
                   dropped_last_iteration=info["normal_angle_dropped"], kept_last_iteration=int(r[-1].n_kept),
                   cache_bytes=info["normal_cache_bytes"], miss_free_iterations_settled=info2["normal_miss_free_iterations"])
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
