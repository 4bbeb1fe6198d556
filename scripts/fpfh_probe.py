"""Measurements of the FPFH descriptors (records under profiles/fpfh/).

    python scripts/fpfh_probe.py [--n 1000000,10000000] [--neighbors 32] [--runs 5] [--out FILE]

For a uniform cloud of each size (already in the slot, its normals estimated into device memory, k = --neighbors): wall time of
Context.fpfh (descriptors into device memory) and, from the library's own event timing (sicp_timing_enable), the part of it that
is the k-NN search -- both passes search, so it is two searches; the rest is pass 1 + pass 2 and the copy of the normals.  Next to
it Context.outlier_statistical at the same k on the same cloud: ONE search plus a trivial epilogue, the natural yardstick.  The
ratio of the two, and the passes' share of HBM peak on algorithmic bytes -- per point and neighbour 36 bytes gathered in pass 1
(coordinates and normal) and 68 in pass 2 (the counts), 16 bytes of list in each, 68 + 132 written per point.  Each after a warm-up,
between device synchronisations, median of --runs.  One JSON line per record; --out appends them to a file.

The split of the rest into pass 1 (k_fpfh_spfh) and pass 2 (k_fpfh_final) is read off a kernel trace, a run of its own:

    timeout -k 10 300 python scripts/fpfh_probe.py --out cost.jsonl && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d trace -o fpfh -- \
        python scripts/fpfh_probe.py --runs 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simpleicp_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="1000000,10000000")
ap.add_argument("--neighbors", type=int, default=32)
ap.add_argument("--runs", type=int, default=5)
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


def timed(ctx, fn, runs):
    """(median wall ms, median ms of the k-NN search inside it, its launches) of fn(), device idle before and after each call"""
    fn()
    torch.cuda.synchronize()
    wall, search, launches = [], [], 0
    for _ in range(runs):
        ctx.timing_reset()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timing()["knnk_scan"]
        search.append(t["ms"])
        launches = t["launches"]
    return float(np.median(wall)), float(np.median(search)), int(launches)


k = args.neighbors
with _lib.Context(0) as ctx:
    for n in (int(v) for v in args.n.split(",")):
        X = torch.rand((n, 3), dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(n)) * (n ** (1.0 / 3.0))
        torch.cuda.synchronize()
        ctx.upload_strided(_lib.FIX, X.data_ptr(), _lib.DT_F64, n, 3, 1)
        sel = torch.arange(n, dtype=torch.int64, device=DEV)
        nv = torch.empty((n, 3), dtype=torch.float32, device=DEV)
        pl = torch.empty(n, dtype=torch.float32, device=DEV)
        out = torch.empty((n, 33), dtype=torch.float32, device=DEV)
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        ctx.estimate_normals_into(_lib.FIX, sel.data_ptr(), n, 10, nv.data_ptr(), pl.data_ptr())
        ctx.timing_enable(True)
        st = ctx.fpfh(_lib.FIX, nv, k, fpfh_ptr=out.data_ptr())
        f_wall, f_search, f_launches = timed(ctx, lambda: ctx.fpfh(_lib.FIX, nv, k, fpfh_ptr=out.data_ptr()), args.runs)
        o_wall, o_search, o_launches = timed(ctx, lambda: ctx.outlier_statistical(_lib.FIX, k, 2.0, keep_ptr=keep.data_ptr()), args.runs)
        ctx.timing_enable(False)
        passes = f_wall - f_search
        bytes_algo = n * ((k - 1) * (36 + 68) + 2 * 16 * k + 68 + 132 + 2 * 12)
        emit(dict(record="fpfh_cost", n=n, neighbors=k, runs=args.runs, fpfh_wall_ms=round(f_wall, 3), fpfh_search_ms=round(f_search, 3),
                  fpfh_search_launches=f_launches, fpfh_passes_ms=round(passes, 3), outlier_wall_ms=round(o_wall, 3),
                  outlier_search_ms=round(o_search, 3), outlier_search_launches=o_launches, ratio_to_outlier=round(f_wall / o_wall, 3),
                  passes_algorithmic_gb=round(bytes_algo / 1e9, 3), passes_gbps=round(bytes_algo / 1e6 / passes, 1),
                  passes_share_of_hbm_peak=round(bytes_algo / 1e6 / passes / HBM_PEAK_GBPS, 4), stats=st.as_dict()))
        del X, sel, nv, pl, out, keep
