"""Times of the DBSCAN labels (records under profiles/cluster/).

    python scripts/cluster_probe.py [--n 100000,1000000,10000000] [--runs 5] [--out FILE]

One JSON line per size of --n; --out appends them to a file.  The cloud is a noisy sample of one smooth surface over [-1, 1]^2, a
float64 device tensor; the radius is the one at which a disc of the plane holds 20 points (sqrt(80 / (pi n))), min_points 10.
On the library's one context, alternating call by call: cluster_labels(X, radius, 10) and outlier_keep(X, radius=radius,
min_points=2**31 - 2) -- the radius filter with a cap no count reaches: ONE uncapped ball walk over every point, the yardstick.
Both calls ingest X first.  Times are wall times between device synchronisations, after a warm-up call of each, the median of --runs.

    timeout -k 10 600 python scripts/cluster_probe.py --out profiles/cluster/probe.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import simpleicp_amd

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100000,1000000,10000000")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
MIN_POINTS = 10


def surface(n):
    g = torch.Generator(DEV).manual_seed(n)
    uv = torch.rand((n, 2), dtype=torch.float64, device=DEV, generator=g) * 2.0 - 1.0
    u, v = uv[:, 0], uv[:, 1]
    z = 0.3 * torch.sin(3 * u) * torch.cos(2 * v) + 0.2 * u * v + 0.05 * torch.sin(11 * u + 7 * v)
    z = z + torch.randn(n, dtype=torch.float64, device=DEV, generator=g) * (0.2 / np.sqrt(n))
    return torch.stack([u, v, z], dim=1).contiguous()


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


for n in (int(v) for v in args.n.split(",") if v):
    X = surface(n)
    radius = float(np.sqrt(80.0 / (np.pi * n)))
    torch.cuda.synchronize()
    cluster = lambda: simpleicp_amd.cluster_labels(X, radius, MIN_POINTS, return_info=True)            # noqa: E731
    walk = lambda: simpleicp_amd.outlier_keep(X, radius=radius, min_points=2**31 - 2)                  # noqa: E731
    once(cluster), once(walk)
    t_cluster, t_walk, info = [], [], None
    for _ in range(args.runs):
        ms, (_, info) = once(cluster)
        t_cluster.append(ms)
        t_walk.append(once(walk)[0])
    rec = dict(record="cluster_cost", n=n, radius=radius, min_points=MIN_POINTS, runs=args.runs,
               cluster_ms=round(float(np.median(t_cluster)), 3), uncapped_walk_ms=round(float(np.median(t_walk)), 3),
               ratio=round(float(np.median(t_cluster) / np.median(t_walk)), 3), cluster_ms_all=[round(t, 3) for t in t_cluster],
               uncapped_walk_ms_all=[round(t, 3) for t in t_walk], stats=info)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del X
