"""Measurements of the least-squares pose refit (records under profiles/posefit/).

    python scripts/posefit_probe.py [--runs 7] [--out FILE]

refine_pose on CUDA tensors at (m, b, rounds) = (400, 8, 3) and (10 000, 64, 3) -- a noisy rigid copy with 40 % wrong matches, the
start poses the true motion off by a few degrees -- and fit_pose at m = 1 000 000 (b = 1, one round).  Next to each the same fit
done with torch in the same process on the same tensors: per round the inlier masks of all poses at once, masked means, the
batched 3 x 3 cross sums, torch.linalg.svd with the determinant fix, then the count of every pose; the best pose is kept as
contract (L) keeps it.  Each after a warm-up, between device synchronisations: wall time of the whole Python call, median,
minimum and maximum of --runs, the two alternating.  The torch fit sums in whatever order its kernels take and is no bit-exact
partner; `agree` is the largest difference between the two sets of poses, `same_counts` whether their inlier counts agree.
One JSON line per record; --out appends them to a file."""
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
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"


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


def torch_count(S, D, R, t, md2):
    d2 = ((S @ R.transpose(1, 2) + t[:, None, :] - D) ** 2).sum(-1)   # (b, m)
    return d2 < md2


def torch_fit(S, D, w):
    """Kabsch of the rows weighted by the masks w (b, m): (R (b, 3, 3), t (b, 3))."""
    n = w.sum(1, keepdim=True).clamp(min=1.0)
    cp, cq = (w @ S) / n, (w @ D) / n
    a, g = S[None] - cp[:, None], D[None] - cq[:, None]
    K = (g * w[:, :, None]).transpose(1, 2) @ a                       # (b, 3, 3): sum of q p^T
    U, _, Vt = torch.linalg.svd(K)
    sign = torch.det(U @ Vt)
    U = torch.cat([U[:, :, :2], U[:, :, 2:] * sign[:, None, None]], dim=2)
    R = U @ Vt
    return R, cq - (R @ cp[:, :, None])[:, :, 0]


def torch_refine(S, D, H, max_distance, rounds):
    md2 = max_distance * max_distance
    R, t = H[:, :3, :3].contiguous(), H[:, :3, 3].contiguous()
    mask = torch_count(S, D, R, t, md2)
    best_R, best_t, best_n = R, t, mask.sum(1)
    for _ in range(rounds):
        R, t = torch_fit(S, D, mask.to(S.dtype))
        mask = torch_count(S, D, R, t, md2)
        n = mask.sum(1)
        better = n > best_n
        best_R = torch.where(better[:, None, None], R, best_R)
        best_t = torch.where(better[:, None], t, best_t)
        best_n = torch.where(better, n, best_n)
    return best_R.cpu().numpy(), best_t.cpu().numpy(), best_n.cpu().numpy()


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])
for m, b, rounds in ((400, 8, 3), (10_000, 64, 3), (1_000_000, 1, 1)):
    rng = np.random.default_rng(m)
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, 0.002, (m, 3))
    plain = b == 1
    if not plain:
        bad = rng.choice(m, int(0.4 * m), replace=False)
        dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    H = np.tile(np.eye(4), (b, 1, 1))
    for k in range(b):
        H[k, :3, :3] = rotation(rng.standard_normal(3), np.radians(3.0) * rng.uniform(0.2, 1.0)) @ R_TRUE
        H[k, :3, 3] = T_TRUE + rng.normal(0, 0.01, 3)
    S, D, Hd = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), torch.tensor(H, device=DEV)
    if plain:
        ones = torch.ones((1, m), dtype=torch.float64, device=DEV)
        ours = lambda: (simpleicp_amd.fit_pose(S, D)[None], np.array([m]))
        theirs = lambda: tuple(x.cpu().numpy() for x in torch_fit(S, D, ones)) + (np.array([m]),)
    else:
        ours = lambda: simpleicp_amd.refine_pose(S, D, H, max_distance=0.05, rounds=rounds)
        theirs = lambda: torch_refine(S, D, Hd, 0.05, rounds)
    (Ho, no), (Rt, tt, nt) = timed(ours)[1], timed(theirs)[1]         # warm-up
    t_ours, t_theirs = [], []
    for _ in range(args.runs):
        t_ours.append(timed(ours)[0])
        t_theirs.append(timed(theirs)[0])
    agree = float(max(np.abs(Ho[:, :3, :3] - Rt).max(), np.abs(Ho[:, :3, 3] - tt).max()))
    emit(dict(what="plain fit" if plain else "refit", m=m, b=b, rounds=rounds, library=spread(t_ours), torch_svd=spread(t_theirs),
              agree=agree, same_counts=bool(np.array_equal(np.asarray(no), nt)),
              rows_per_s=float(m) * b * (2 * rounds + 1) / (np.median(t_ours) * 1e-3)))
