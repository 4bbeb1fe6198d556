"""Times of the plane segmentation (records under profiles/plane/).

    python scripts/plane_probe.py [--n 100000,1000000,10000000] [--h 1024] [--runs 7] [--out FILE]

One JSON line per size of --n; --out appends them to a file.  The cloud is a float64 device tensor: 60 % of its rows a tilted
plane with 1 cm of noise in a 20 m cube, the rest uniform clutter; max_distance 0.05; the triples are drawn on the host from
seed 0.  Per size, on the library's one context, after a warm-up call of each, --runs runs of
  triplets   sicp_plane_triplets, device rows, host triples and outputs (the whole call, its copies and its record included)
  refit      sicp_plane_refit of the best plane, b = 1, rounds = 3, keep_out on the device (sizes from 1 000 000 on)
  torch      the same counts in torch float64: ((X @ N.T + d).abs() < t).sum(0), 65 536 rows at a time
  read       X.sum(): one pass over the cloud, the streaming rate the blocking is held against
as wall times between device synchronisations: median, minimum and maximum.  `bound_read_ms` is the time to read the cloud once
per hypothesis block (512 hypotheses a block from 257 on, else 256) at the measured rate.

    timeout -k 10 500 python scripts/plane_probe.py --out profiles/plane/probe.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simpleicp_amd import backend
from simpleicp_amd.tensors import _wait_for_torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100000,1000000,10000000")
ap.add_argument("--h", type=int, default=1024)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
MD = 0.05


def scene(n):
    g = torch.Generator(DEV).manual_seed(n)
    k = (3 * n) // 5
    X = torch.rand((n, 3), dtype=torch.float64, device=DEV, generator=g) * 20.0 - 10.0
    X[:k, 2] = 0.2 * X[:k, 0] - 0.3 * X[:k, 1] + 1.5 + (torch.rand(k, dtype=torch.float64, device=DEV, generator=g) - 0.5) * 0.02
    return X[torch.randperm(n, device=DEV, generator=g)].contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def series(fn, runs):
    timed(fn)
    t = [timed(fn)[0] for _ in range(runs)]
    return dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))


ctx = backend.get_context()
for n in (int(v) for v in args.n.split(",") if v):
    X = scene(n)
    h = args.h
    tri = np.random.default_rng(0).integers(0, n, (h, 3), dtype=np.int32)
    planes, inl = np.empty((h, 4)), np.empty(h, np.int32)
    _wait_for_torch(ctx, X.device)

    def triplets():
        return ctx.plane_triplets(X.data_ptr(), tri.ctypes.data, MD, n=n, h=h, planes_ptr=planes.ctypes.data, inliers_ptr=inl.ctypes.data)

    st = triplets().as_dict()
    rec = dict(record="plane_cost", n=n, h=h, max_distance=MD, runs=args.runs, stats=st, triplets_ms=series(triplets, args.runs))
    N = torch.from_numpy(planes[:, :3].copy()).to(DEV)
    d = torch.from_numpy(planes[:, 3].copy()).to(DEV)

    def in_torch():
        cnt = torch.zeros(h, dtype=torch.int64, device=DEV)
        for lo in range(0, n, 65536):
            cnt += ((X[lo:lo + 65536] @ N.T + d).abs() < MD).sum(0)
        return cnt

    rec["torch_ms"] = series(in_torch, max(3, args.runs // 2))
    valid = inl >= 0
    rec["torch_counts_differ"] = int((in_torch().cpu().numpy()[valid] != inl[valid]).sum())      # (another rounding: a handful may)
    rec["read_ms"] = series(lambda: X.sum(), args.runs)
    rate = 24.0 * n / (rec["read_ms"]["median"] * 1e-3)
    blocks = -(-h // (512 if h > 256 else 256))
    rec["read_GBps"] = round(rate / 1e9, 1)
    rec["bound_read_ms"] = round(24.0 * n * blocks / rate * 1e3, 3)
    rec["residuals_per_s"] = round(float(n) * (h - st["n_void"]) / (rec["triplets_ms"]["median"] * 1e-3), 1)
    if n >= 1_000_000:
        start = np.ascontiguousarray(planes[st["best"]:st["best"] + 1])
        out, cnt = np.empty((1, 4)), np.empty(1, np.int32)
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        _wait_for_torch(ctx, X.device)

        def refit():
            return ctx.plane_refit(X.data_ptr(), start.ctypes.data, MD, 3, n=n, b=1, planes_ptr=out.ctypes.data, inliers_ptr=cnt.ctypes.data,
                                   keep_ptr=keep.data_ptr())

        rec["refit_stats"] = refit().as_dict()
        rec["refit_ms"] = series(refit, args.runs)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del X
