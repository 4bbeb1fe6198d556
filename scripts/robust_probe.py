"""Measurements of the robust pose fit (records under profiles/robust/).

    python scripts/robust_probe.py [--runs 7] [--out FILE]

robust_pose's call (Context.pose_robust on device pointers, the automatic scale, divisor 1.4, max_distance 0.01) at (m, b,
rounds) = (400, 1, 64), (4 096, 8, 64) and (1 000 000, 1, 40) -- a noisy rigid copy with 60 % wrong matches, the starts the
identity and the true motion off by up to 20 degrees -- on a context per path of sicp_pose_robust (SICP_ROBUST=sweeps, =one; the
one-launch path applies up to 16 384 rows).  Next to each the same iteration done with torch in the same process on the same
tensors: per round the weights of all poses at once, weighted means, the batched 3 x 3 cross sums, torch.linalg.svd with the
determinant fix; then the count of every pose.  Each after a warm-up, between device synchronisations: wall time of the whole
Python call, median, minimum and maximum of --runs, the three alternating.  The torch fit sums in whatever order its kernels take
and is no bit-exact partner; `agree` is the largest difference between its poses and the library's, `same_bits` whether the two
paths of the library agree bit for bit.  One JSON line per record; --out appends them to a file."""
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
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
ONE_MAX = 16384


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def forced(path):
    os.environ["SICP_ROBUST"] = path                                  # (read at sicp_ctx_create)
    try:
        return _lib.Context(0)
    finally:
        del os.environ["SICP_ROBUST"]


def torch_d2(S, D, R, t):
    return ((S @ R.transpose(1, 2) + t[:, None, :] - D) ** 2).sum(-1)  # (b, m)


def torch_robust(S, D, poses, max_distance, rounds, divisor):
    md2 = max_distance * max_distance
    R, t = poses[:, :9].reshape(-1, 3, 3).contiguous(), poses[:, 9:].contiguous()
    s = (2.0 * torch_d2(S, D, R, t).max(dim=1).values).clamp(min=md2)
    for _ in range(rounds):
        w = (s[:, None] / (s[:, None] + torch_d2(S, D, R, t))) ** 2
        W = w.sum(1, keepdim=True)
        cp, cq = (w @ S) / W, (w @ D) / W
        a, g = S[None] - cp[:, None], D[None] - cq[:, None]
        K = (g * w[:, :, None]).transpose(1, 2) @ a                   # (b, 3, 3): sum of w q p^T
        U, _, Vt = torch.linalg.svd(K)
        sign = torch.det(U @ Vt)
        U = torch.cat([U[:, :, :2], U[:, :, 2:] * sign[:, None, None]], dim=2)
        R = U @ Vt
        t = cq - (R @ cp[:, :, None])[:, :, 0]
        s = (s / divisor).clamp(min=md2)
    n = (torch_d2(S, D, R, t) < md2).sum(1)
    return torch.cat([R.reshape(-1, 9), t], dim=1).cpu().numpy(), n.cpu().numpy()


def library(ctx, S, D, poses, m, b, rounds):
    out, inl, scales = np.empty((b, 12)), np.empty(b, np.int32), np.empty(b)
    ctx.pose_robust(S.data_ptr(), D.data_ptr(), poses.ctypes.data, 0.01, rounds, 1.4, 0.0, m=m, b=b, poses_ptr=out.ctypes.data,
                    inliers_ptr=inl.ctypes.data, scales_ptr=scales.ctypes.data)
    return out, inl, scales


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])
ctxs = {"sweeps": forced("sweeps"), "one": forced("one")}
for m, b, rounds in ((400, 1, 64), (4096, 8, 64), (1_000_000, 1, 40)):
    rng = np.random.default_rng(m)
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, 0.002, (m, 3))
    bad = rng.choice(m, int(0.6 * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    poses = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (b, 1))
    for k in range(1, b):
        poses[k, :9] = (rotation(rng.standard_normal(3), np.radians(20.0) * rng.uniform(0.2, 1.0)) @ R_TRUE).ravel()
        poses[k, 9:] = T_TRUE + rng.normal(0, 0.05, 3)
    S, D, Pd = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), torch.tensor(poses, device=DEV)
    calls = {name: (lambda c=c: library(c, S, D, poses, m, b, rounds)) for name, c in ctxs.items() if name == "sweeps" or m <= ONE_MAX}
    calls["torch_svd"] = lambda: torch_robust(S, D, Pd, 0.01, rounds, 1.4)
    first = {name: timed(fn)[1] for name, fn in calls.items()}         # warm-up
    times = {name: [] for name in calls}
    for _ in range(args.runs):
        for name, fn in calls.items():
            times[name].append(timed(fn)[0])
    rec = dict(what="robust fit", m=m, b=b, rounds=rounds, inliers=first["sweeps"][1].tolist(), torch_inliers=first["torch_svd"][1].tolist(),
               agree=float(np.abs(first["sweeps"][0] - first["torch_svd"][0]).max()))
    if "one" in first:
        rec["same_bits"] = bool(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first["sweeps"], first["one"])))
    rec.update({name: spread(ms) for name, ms in times.items()})
    emit(rec)
