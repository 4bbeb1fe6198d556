"""Measurements of the ISS keypoints (records under profiles/keypoints/).

    python scripts/keypoints_probe.py [--n 100000,1000000,10000000] [--pair 100000] [--runs 5] [--out FILE]

Three kinds of record, one JSON line each; --out appends them to a file.  Times are wall times between device synchronisations,
after a warm-up call, the median of --runs.

  keypoints_cost   a uniform cloud of each size of --n, already in the slot: Context.keypoints at the defaults of keypoint_keep
                   (neighbors 32, no radius), verdicts into device memory; next to it, from the library's own event timing, the part
                   that is the k-NN search (pass 1 searches every point, pass 2 the salient ones), and Context.outlier_statistical
                   at the same k: ONE search of every point, the yardstick.
  global_pair      register_global on two noisy samples of --pair points of one smooth surface, device tensors, with and without
                   keypoints=True: wall time, matches, inliers, and the error against the motion that made the pair.
  bunny_chain      the bunny pair of tests/test_gpu_global.py (1 500 points a cloud) with and without keypoints (neighbors 32,
                   nms_neighbors 6, the parameters of tests/test_keypoints_host.py): rotation and translation error, robust method.

    timeout -k 10 600 python scripts/keypoints_probe.py --out profiles/keypoints/probe.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import simpleicp_amd
from simpleicp_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100000,1000000,10000000")
ap.add_argument("--pair", type=int, default=100000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
K = 32


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, runs, ctx=None):
    """(median wall ms, median ms of the k-NN search inside it) of fn(), the device idle before and after each call"""
    fn()
    torch.cuda.synchronize()
    wall, search = [], []
    for _ in range(runs):
        if ctx is not None:
            ctx.timing_reset()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if ctx is not None:
            search.append(ctx.timing()["knnk_scan"]["ms"])
    return float(np.median(wall)), (float(np.median(search)) if search else None)


def pose_error(H, R, t):
    """(degrees, length) between H and the inverse of the motion (R, t) that made the movable cloud"""
    Rt, tt = R.T, -R.T @ t
    dR = H[:3, :3] @ Rt.T
    return float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))), float(np.linalg.norm(H[:3, 3] - tt))


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


with _lib.Context(0) as ctx:
    for n in (int(v) for v in args.n.split(",") if v):
        X = torch.rand((n, 3), dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(n)) * (n ** (1.0 / 3.0))
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        ctx.upload_strided(_lib.FIX, X.data_ptr(), _lib.DT_F64, n, 3, 1)
        ctx.timing_enable(True)
        st = ctx.keypoints(_lib.FIX, K, keep_ptr=keep.data_ptr())
        k_wall, k_search = timed(lambda: ctx.keypoints(_lib.FIX, K, keep_ptr=keep.data_ptr()), args.runs, ctx)
        o_wall, o_search = timed(lambda: ctx.outlier_statistical(_lib.FIX, K, 2.0, keep_ptr=keep.data_ptr()), args.runs, ctx)
        ctx.timing_enable(False)
        emit(dict(record="keypoints_cost", n=n, neighbors=K, runs=args.runs, keypoints_wall_ms=round(k_wall, 3),
                  keypoints_search_ms=round(k_search, 3), keypoints_passes_ms=round(k_wall - k_search, 3), outlier_wall_ms=round(o_wall, 3),
                  outlier_search_ms=round(o_search, 3), ratio_to_outlier=round(k_wall / o_wall, 3), stats=st.as_dict()))
        del X, keep

if args.pair > 0:
    rng = np.random.default_rng(args.pair)

    def surface(m):
        u, v = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
        z = 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * u * v + 0.05 * np.sin(11 * u + 7 * v)
        return np.column_stack([u, v, z]) + rng.normal(0, 2e-4, (m, 3))

    R, t = rotation((1.0, 2.0, 3.0), 0.7), np.array([0.5, 0.1, -0.4])
    A, B = surface(args.pair), surface(args.pair) @ R.T + t
    vA = np.array([0.0, 0.0, 9.0])
    At, Bt = torch.tensor(A, device=DEV), torch.tensor(B, device=DEV)
    kw = dict(max_distance=0.01, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(R @ vA + t), method="robust")
    for name, extra in (("all points", {}), ("keypoints=True", dict(keypoints=True))):
        res = simpleicp_amd.register_global(At, Bt, **extra, **kw)
        wall, _ = timed(lambda: simpleicp_amd.register_global(At, Bt, **extra, **kw), args.runs)
        angle, shift = pose_error(res.H, R, t) if res.H is not None else (None, None)
        emit(dict(record="global_pair", n=args.pair, chain=name, method="robust", runs=args.runs, wall_ms=round(wall, 3),
                  n_keypoints=res.n_keypoints, n_matches=res.n_matches, inliers=res.inliers, rotation_error_deg=angle, translation_error=shift))

EXTENT = 263_800.0
X = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "data", "bunny_part1.npz"))["q"].astype(np.float64)
perm = np.random.default_rng(1).permutation(len(X))
A = np.ascontiguousarray(X[perm[:1500]])
R, t = rotation((1.0, 2.0, 3.0), 0.7), np.array([0.05, -0.02, 0.1]) * EXTENT
B = np.ascontiguousarray(X[perm[1500:3000]] @ R.T + t)
vA = A.mean(axis=0) + np.array([0.0, 0.0, 2_638_000.0])
kw = dict(max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(R @ vA + t), method="robust")
for name, extra in (("all points", {}), ("keypoints", dict(keypoints=dict(neighbors=32, nms_neighbors=6)))):
    res = simpleicp_amd.register_global(A, B, **extra, **kw)
    angle, shift = pose_error(res.H, R, t) if res.H is not None else (None, None)
    emit(dict(record="bunny_chain", chain=name, method="robust", n_keypoints=res.n_keypoints, n_matches=res.n_matches, inliers=res.inliers,
              rotation_error_deg=angle, translation_error_of_extent=None if shift is None else shift / EXTENT))
