"""Times of the smooth regions (records under profiles/regions/).

    python scripts/regions_probe.py [--n 100000,1000000,10000000] [--runs 5] [--host 100000,1000000] [--out FILE]

Per size a surface-like cloud (a wavy height field, its analytic normals with noise) as CUDA tensors, generated on the device.
On the library's one context, alternating call by call: smooth_regions(X, N, neighbors=16, max_angle=8), outlier_keep(X,
neighbors=16) -- one k-NN pass of the same k, the yardstick of profiles/orient/ -- and orient_normals(X, N, neighbors=16) on the
same cloud; wall clock around each call with a device synchronisation behind it, medians of --runs.  `knn_ms` is the k-NN's part
of one regions call by the library's own events (sicp_timing_get).

--host: the same labels on the host at these sizes, for outside scale -- a cKDTree for the lists, numpy for the agreement,
scipy.sparse.csgraph.connected_components for the regions (no seeds, no border points: all points are smooth here).

On a shared machine give the run a time limit of its own:
    timeout -k 10 900 python scripts/regions_probe.py --out profiles/regions/probe.jsonl"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import simpleicp_amd
from simpleicp_amd import backend

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100000,1000000,10000000")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
K = 16
ANGLE = 8.0


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def surface(n):
    g = torch.Generator(DEV).manual_seed(n)
    uv = torch.rand((n, 2), dtype=torch.float64, device=DEV, generator=g) * 2.0 - 1.0
    u, v = uv[:, 0], uv[:, 1]
    z = 0.3 * torch.sin(3 * u) * torch.cos(2 * v) + 0.2 * u * v
    zu = 0.9 * torch.cos(3 * u) * torch.cos(2 * v) + 0.2 * v
    zv = -0.6 * torch.sin(3 * u) * torch.sin(2 * v) + 0.2 * u
    N = torch.stack([-zu, -zv, torch.ones_like(zu)], dim=1)
    N = N / N.norm(dim=1, keepdim=True) + torch.randn((n, 3), dtype=torch.float64, device=DEV, generator=g) * 0.05
    N = (N / N.norm(dim=1, keepdim=True)).to(torch.float32).contiguous()
    z = z + torch.randn(n, dtype=torch.float64, device=DEV, generator=g) * (0.2 / np.sqrt(n))
    return torch.stack([u, v, z], dim=1).contiguous(), N


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_regions(X, N, cos_min):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    n = len(X)
    idx = cKDTree(X).query(X, k=K)[1]
    i, j = np.repeat(np.arange(n), K), idx.ravel()
    link = np.abs((N[i] * N[j]).sum(axis=1)) >= cos_min
    count, _ = connected_components(coo_matrix((np.ones(int(link.sum()), np.int8), (i[link], j[link])), shape=(n, n)), directed=False)
    return (time.perf_counter() - t0) * 1e3, int(count)


for n in (int(v) for v in args.n.split(",") if v):
    X, N = surface(n)
    torch.cuda.synchronize()
    regions = lambda: simpleicp_amd.smooth_regions(X, N, neighbors=K, max_angle=ANGLE, return_info=True)   # noqa: E731
    knn = lambda: simpleicp_amd.outlier_keep(X, neighbors=K)                                              # noqa: E731
    orient = lambda: simpleicp_amd.orient_normals(X, N, neighbors=K)                                      # noqa: E731
    once(regions), once(knn), once(orient)
    t_regions, t_knn, t_orient, info = [], [], [], None
    for _ in range(args.runs):
        ms, (_, info) = once(regions)
        t_regions.append(ms)
        t_knn.append(once(knn)[0])
        t_orient.append(once(orient)[0])
    ctx = backend.get_context()
    ctx.timing_enable(True)
    ctx.timing_reset()
    once(regions)
    knn_ms = ctx.timing()
    ctx.timing_enable(False)
    med = lambda t: float(np.median(t))                                                                   # noqa: E731
    emit(dict(record="regions_cost", n=n, k=K, max_angle=ANGLE, runs=args.runs, regions_ms=round(med(t_regions), 3),
              one_knn_pass_ms=round(med(t_knn), 3), orient_ms=round(med(t_orient), 3), ratio=round(med(t_regions) / med(t_knn), 3),
              regions_over_orient=round(med(t_regions) / med(t_orient), 3), regions_ms_all=[round(t, 3) for t in t_regions],
              one_knn_pass_ms_all=[round(t, 3) for t in t_knn], orient_ms_all=[round(t, 3) for t in t_orient],
              knn_ms={name: round(v["ms"], 3) for name, v in knn_ms.items() if v["launches"]}, stats=info))
    if str(n) in args.host.split(","):
        ms, count = host_regions(X.cpu().numpy(), N.cpu().numpy().astype(np.float64), math.cos(math.radians(ANGLE)))
        emit(dict(record="regions_host_scipy", n=n, k=K, ms=round(ms, 1), n_regions_all=count, library_n_regions_all=info["n_regions_all"]))
    del X, N
