"""Measurements of the match consistency operator (records under profiles/consistency/).

    python scripts/consistency_probe.py [--runs 7] [--out FILE] [--sizes 400,4096,32768]

consistent_matches' call (Context.match_consistency on device pointers, tolerance 0.01, min_length 0.1) on a noisy rigid copy of m
rows with 60 % and with 95 % wrong matches, on a context per path of the peeling (SICP_CONSISTENCY=sweeps, =one; the one-launch
path applies up to 4 096 rows).  Next to each the same work done with torch in the same process on the same tensors: the dense
boolean matrix from two torch.cdist calls in float64, the degrees as its row sums, the same peel (the level jumps to the smallest
remaining degree) with tensor operations and one .item() per pass.  Each after a warm-up, between device synchronisations: wall
time of the whole Python call, median, minimum and maximum of --runs, the callers alternating.  The torch restatement is a
yardstick nobody tuned; its lengths are rounded as torch.cdist rounds them (through a matrix product from 26 rows on), so a pair
at the threshold may fall on the other side:
`torch_differs` is the number of rows whose core number differs from the library's, `same` whether the two paths of the library
agree exactly.  One JSON line per record; --out appends them to a file."""
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
ap.add_argument("--sizes", default="400,4096,32768")
args = ap.parse_args()
DEV = "cuda:0"
ONE_MAX = 4096
TOLERANCE, MIN_LENGTH = 0.01, 0.1


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
    os.environ["SICP_CONSISTENCY"] = path                             # (read at sicp_ctx_create)
    try:
        return _lib.Context(0)
    finally:
        del os.environ["SICP_CONSISTENCY"]


def torch_consistency(S, D):
    a, b = torch.cdist(S, S), torch.cdist(D, D)
    A = ((a - b).abs() <= TOLERANCE) & (a >= MIN_LENGTH) & (b >= MIN_LENGTH)
    del a, b
    A.fill_diagonal_(False)
    degree = A.sum(1, dtype=torch.int32)
    work, alive, core = degree.clone(), torch.ones_like(degree, dtype=torch.bool), torch.zeros_like(degree)
    k = 0
    while True:
        left = work[alive]
        if left.numel() == 0:
            break
        k = max(k, int(left.min().item()))
        front = alive & (work <= k)
        core[front] = k
        alive &= ~front
        work -= A[:, front].sum(1, dtype=torch.int32)
    return degree, core


def library(ctx, S, D, m):
    degree = torch.empty(m, dtype=torch.int32, device=DEV)
    core = torch.empty(m, dtype=torch.int32, device=DEV)
    st = ctx.match_consistency(S.data_ptr(), D.data_ptr(), TOLERANCE, MIN_LENGTH, m=m, degree_ptr=degree.data_ptr(), core_ptr=core.data_ptr())
    return degree, core, st.as_dict()


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])
ctxs = {"sweeps": forced("sweeps"), "one": forced("one")}
for m in (int(v) for v in args.sizes.split(",")):
    for wrong in (0.6, 0.95):
        rng = np.random.default_rng(m)
        src = rng.uniform(-1, 1, (m, 3))
        dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, 0.002, (m, 3))
        bad = rng.choice(m, int(wrong * m), replace=False)
        dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
        S, D = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV)
        calls = {name: (lambda c=c: library(c, S, D, m)) for name, c in ctxs.items() if name == "sweeps" or m <= ONE_MAX}
        calls["torch"] = lambda: torch_consistency(S, D)
        first = {name: timed(fn)[1] for name, fn in calls.items()}     # warm-up
        times = {name: [] for name in calls}
        for _ in range(args.runs):
            for name, fn in calls.items():
                times[name].append(timed(fn)[0])
        stats = first["sweeps"][2]
        rec = dict(what="match consistency", m=m, wrong=wrong, right=m - len(bad), stats=stats,
                   torch_differs=int((first["sweeps"][1] != first["torch"][1]).sum().item()))
        if "one" in first:
            rec["same"] = bool(torch.equal(first["sweeps"][0], first["one"][0]) and torch.equal(first["sweeps"][1], first["one"][1]))
            rec["one_subrounds"] = first["one"][2]["n_subrounds"]
        rec.update({name: spread(ms) for name, ms in times.items()})
        emit(rec)
