"""Times of the consistent normal orientation (records under profiles/orient/).

    python scripts/orient_probe.py [--n 100000,1000000,10000000] [--runs 5] [--host 100000,1000000] [--bunny] [--out FILE]

One JSON line per size of --n; --out appends them to a file.  The cloud is a noisy sample of one smooth surface over [-1, 1]^2, a
float64 device tensor, its normals the surface's own, each negated by a seeded coin (float32 on the device: "normals given").
On the library's one context, alternating call by call: orient_normals(X, N, neighbors=16, away_from=...) and
outlier_keep(X, neighbors=16) -- the statistical filter: ONE k-NN pass of the same k over every point, the yardstick: the lists are
the floor of the operator, the ratio says what the forest costs on top of them.  Both calls ingest X first.  Times are wall times
between device synchronisations, after a warm-up call of each, the median of --runs; `knn_ms` is the k-NN search's share of one
orient call by the library's own events (sicp_timing_get), `rounds` comes from the call's record.

--host: the same orientation on the host at these sizes, for outside scale -- scipy.sparse.csgraph.minimum_spanning_tree over
1 - |dot| on a scipy cKDTree's lists, then a breadth-first walk (one run; its forest differs from the contract's in ties).
--bunny: register_global on the bundled bunny pair three ways -- viewpoints as before, orient=16 with the same viewpoints as vote,
orient=16 without a viewpoint -- with n_matches, inliers and the pose's error against the known truth.

    timeout -k 10 900 python scripts/orient_probe.py --bunny --out profiles/orient/probe.jsonl"""
import argparse
import json
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
ap.add_argument("--bunny", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
K = 16


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
    coin = torch.rand(n, device=DEV, generator=g) < 0.5
    N = torch.where(coin[:, None], -N, N).to(torch.float32).contiguous()
    z = z + torch.randn(n, dtype=torch.float64, device=DEV, generator=g) * (0.2 / np.sqrt(n))
    return torch.stack([u, v, z], dim=1).contiguous(), N


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_orientation(X, N):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import breadth_first_order, minimum_spanning_tree
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    n = len(X)
    idx = cKDTree(X).query(X, k=K)[1]
    i, j = np.repeat(np.arange(n), K), idx.ravel()
    w = 1.0 - np.abs((N[i] * N[j]).sum(axis=1)) + 1e-12
    T = minimum_spanning_tree(coo_matrix((w, (i, j)), shape=(n, n)).tocsr())
    T = T + T.T
    order, pred = breadth_first_order(T, 0, directed=False)
    flip = np.zeros(n, bool)
    for v in order[1:]:
        flip[v] = flip[pred[v]] ^ bool((N[v] * N[pred[v]]).sum() < 0.0)
    return (time.perf_counter() - t0) * 1e3, int(len(order))


for n in (int(v) for v in args.n.split(",") if v):
    X, N = surface(n)
    away = (0.0, 0.0, -10.0)
    torch.cuda.synchronize()
    orient = lambda: simpleicp_amd.orient_normals(X, N, neighbors=K, away_from=away, return_info=True)   # noqa: E731
    knn = lambda: simpleicp_amd.outlier_keep(X, neighbors=K)                                            # noqa: E731
    once(orient), once(knn)
    t_orient, t_knn, info = [], [], None
    for _ in range(args.runs):
        ms, (_, info) = once(orient)
        t_orient.append(ms)
        t_knn.append(once(knn)[0])
    ctx = backend.get_context()
    ctx.timing_enable(True)
    ctx.timing_reset()
    once(orient)
    knn_ms = ctx.timing()
    ctx.timing_enable(False)
    emit(dict(record="orient_cost", n=n, k=K, runs=args.runs, orient_ms=round(float(np.median(t_orient)), 3),
              one_knn_pass_ms=round(float(np.median(t_knn)), 3), ratio=round(float(np.median(t_orient) / np.median(t_knn)), 3),
              orient_ms_all=[round(t, 3) for t in t_orient], one_knn_pass_ms_all=[round(t, 3) for t in t_knn],
              knn_ms={name: round(v["ms"], 3) for name, v in knn_ms.items() if v["launches"]}, rounds=info["rounds"], stats=info))
    if str(n) in args.host.split(","):
        ms, reached = host_orientation(X.cpu().numpy(), N.cpu().numpy().astype(np.float64))
        emit(dict(record="orient_host_scipy", n=n, k=K, ms=round(ms, 1), reached=reached))
    del X, N

if args.bunny:
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "data")
    fix = np.load(os.path.join(d, "bunny_part1.npz"))["q"].astype(np.float64)
    rng = np.random.default_rng(1)
    a = 0.6
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.ptp(fix, axis=0) * np.array([0.5, -0.3, 0.2])
    keep = rng.random(len(fix)) < 0.7                                  # the movable cloud: 70 % of the same scan, moved by a known pose
    mov = np.ascontiguousarray((fix[keep] - t) @ R)                    # so that fixed = R @ movable + t
    size = float(np.ptp(fix, axis=0).max())
    vf = fix.mean(axis=0) + np.array([0.0, 0.0, 3.0 * size])
    vm = (vf - t) @ R
    ways = (("viewpoints", dict(viewpoint_fixed=vf, viewpoint_movable=vm)),
            ("orient=16, viewpoints as vote", dict(viewpoint_fixed=vf, viewpoint_movable=vm, orient=16)),
            ("orient=16, no viewpoint", dict(orient=16)))
    for name, kw in ways:
        res = simpleicp_amd.register_global(fix, mov, max_distance=size / 50.0, seed=3, **kw)
        err_R = err_t = None
        if res.H is not None:
            err_R = float(np.degrees(np.arccos(np.clip((np.trace(res.H[:3, :3].T @ R) - 1.0) / 2.0, -1.0, 1.0))))
            err_t = float(np.linalg.norm(res.H[:3, 3] - t) / size)
        emit(dict(record="register_global_bunny", way=name, n_fixed=len(fix), n_movable=len(mov), n_matches=res.n_matches,
                  inliers=res.inliers, rotation_error_deg=err_R, translation_error_over_size=err_t, n_components=res.n_components))
