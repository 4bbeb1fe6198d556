"""Measurements of descriptor matching and RANSAC poses (records under profiles/global/).

    python scripts/global_probe.py [--runs 5] [--big 1000000] [--out FILE]

match_features on 33-wide float32 rows in device memory against what the README recommended before
(torch.cdist(q, t).argmin(1), same process, same tensors) at 10 k x 10 k and 50 k x 50 k, where cdist's matrix still fits, and
alone at --big x --big (0: skipped).  ransac_pose at (m, h) = (2 000, 10 000) and (10 000, 100 000) on a noisy rigid copy with
40 % wrong matches, triples drawn once.  Each after a warm-up, between device synchronisations; median, minimum and maximum of
--runs, the two matchers alternating.  The matching kernel's share of the FP32 vector peak counts 3 x dim flop per pair over the
call's wall time (a lower bound of the kernel's own share; without FMA, one flop per lane and instruction, half the peak is the
ceiling).  One JSON line per record; --out appends them to a file."""
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
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--big", type=int, default=1_000_000)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"
FP32_VECTOR_PEAK_TFLOPS = 157.3
DIM = 33


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


def rows(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((n, DIM), device=DEV, generator=g) * 200.0


for n in (10_000, 50_000):
    q, t = rows(n, 1), rows(n, 2)
    ours = lambda: simpleicp_amd.match_features(q, t)
    theirs = lambda: torch.cdist(q, t).argmin(1)
    a, b = timed(ours)[1], timed(theirs)[1]                           # warm-up
    t_ours, t_theirs = [], []
    for _ in range(args.runs):
        t_ours.append(timed(ours)[0])
        t_theirs.append(timed(theirs)[0])
    flop = 3.0 * DIM * n * n
    emit(dict(what="match", nq=n, nt=n, dim=DIM, match_features=spread(t_ours), cdist_argmin=spread(t_theirs),
              agree=float((a == b).float().mean()), tflops=flop / (np.median(t_ours) * 1e-3) / 1e12,
              share_of_fp32_vector_peak=flop / (np.median(t_ours) * 1e-3) / 1e12 / FP32_VECTOR_PEAK_TFLOPS))
    del a, b
if args.big:
    n = args.big
    q, t = rows(n, 3), rows(n, 4)
    ours = lambda: simpleicp_amd.match_features(q, t)
    timed(lambda: simpleicp_amd.match_features(q[:4096], t[:4096]))   # warm-up (code objects, scratch)
    ms = [timed(ours)[0] for _ in range(min(args.runs, 3))]
    flop = 3.0 * DIM * n * n
    emit(dict(what="match", nq=n, nt=n, dim=DIM, match_features=spread(ms), cdist_argmin=None,
              tflops=flop / (np.median(ms) * 1e-3) / 1e12,
              share_of_fp32_vector_peak=flop / (np.median(ms) * 1e-3) / 1e12 / FP32_VECTOR_PEAK_TFLOPS))
    del q, t
for m, h in ((2_000, 10_000), (10_000, 100_000)):
    rng = np.random.default_rng(m)
    src = rng.uniform(-1, 1, (m, 3))
    c, s = np.cos(0.7), np.sin(0.7)
    dst = src @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + 0.1 + rng.normal(0, 0.002, (m, 3))
    bad = rng.choice(m, int(0.4 * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    S, D = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV)
    tri = rng.integers(0, m, (h, 3), dtype=np.int32)
    run = lambda: simpleicp_amd.ransac_pose(S, D, max_distance=0.02, triples=tri)
    res = timed(run)[1]
    ms = [timed(run)[0] for _ in range(args.runs)]
    scored = h - res.stats["n_void"] - res.stats["n_pruned"]
    emit(dict(what="ransac", m=m, h=h, ransac_pose=spread(ms), stats=res.stats, scored_pairs=scored * m,
              gpairs_per_s=scored * m / (np.median(ms) * 1e-3) / 1e9))
