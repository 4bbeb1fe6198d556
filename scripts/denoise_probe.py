"""Times of the moving-least-squares smoothing (records under profiles/denoise/).

    python scripts/denoise_probe.py [--n 100000,1000000,10000000] [--runs 5] [--host 100000,1000000] [--out FILE]

Per size a surface-like cloud (a wavy height field with noise) as a CUDA tensor, generated on the device.  On the library's one
context, alternating call by call: denoise_points(X, neighbors=16) and outlier_keep(X, neighbors=16) -- one k-NN pass of the same
k, the yardstick of profiles/orient/ and profiles/regions/; wall clock around each call with a device synchronisation behind it,
medians of --runs.  `knn_ms` is the k-NN's part of one denoise call by the library's own events (sicp_timing_get); `project_ms`
is what is left of that call's median: the projection kernel, the upload and the launches.  The residual against the clean
surface before and after the call goes into the record.

--host: the same projection on the host at these sizes -- a cKDTree for the lists, numpy for the centred sums, np.linalg.eigh for
the planes -- with the largest coordinate difference from the library's result.

On a shared machine give the run a time limit of its own:
    timeout -k 10 900 python scripts/denoise_probe.py --out profiles/denoise/probe.jsonl"""
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
    sigma = 0.5 / np.sqrt(n)                                          # (a quarter of the mean point spacing)
    clean = torch.stack([u, v, z], dim=1).contiguous()
    return (clean + torch.randn((n, 3), dtype=torch.float64, device=DEV, generator=g) * torch.tensor([0.0, 0.0, sigma], device=DEV,
                                                                                                    dtype=torch.float64)).contiguous(), sigma


def height(P):
    return 0.3 * torch.sin(3 * P[:, 0]) * torch.cos(2 * P[:, 1]) + 0.2 * P[:, 0] * P[:, 1]


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_mls(X):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    idx = cKDTree(X).query(X, k=K)[1]
    P = X[idx]
    c = P.mean(axis=1)
    d = P - c[:, None, :]
    nv = np.linalg.eigh(np.einsum("nka,nkb->nab", d, d) / K)[1][:, :, 0]
    out = X - np.einsum("na,na->n", X - c, nv)[:, None] * nv
    return (time.perf_counter() - t0) * 1e3, out


for n in (int(v) for v in args.n.split(",") if v):
    X, sigma = surface(n)
    torch.cuda.synchronize()
    denoise = lambda: simpleicp_amd.denoise_points(X, neighbors=K, return_info=True)   # noqa: E731
    knn = lambda: simpleicp_amd.outlier_keep(X, neighbors=K)                           # noqa: E731
    once(denoise), once(knn)
    t_denoise, t_knn, out, info = [], [], None, None
    for _ in range(args.runs):
        ms, (out, info) = once(denoise)
        t_denoise.append(ms)
        t_knn.append(once(knn)[0])
    ctx = backend.get_context()
    ctx.timing_enable(True)
    ctx.timing_reset()
    once(denoise)
    knn_ms = {name: round(v["ms"], 3) for name, v in ctx.timing().items() if v["launches"]}
    ctx.timing_enable(False)
    med = lambda t: float(np.median(t))                                                # noqa: E731
    inner = (X[:, :2].abs() < 0.9).all(dim=1)
    before = float((X[inner, 2] - height(X[inner])).square().mean().sqrt())
    after = float((out[inner, 2] - height(out[inner])).square().mean().sqrt())
    emit(dict(record="denoise_cost", n=n, k=K, runs=args.runs, denoise_ms=round(med(t_denoise), 3), one_knn_pass_ms=round(med(t_knn), 3),
              ratio=round(med(t_denoise) / med(t_knn), 3), denoise_ms_all=[round(t, 3) for t in t_denoise],
              one_knn_pass_ms_all=[round(t, 3) for t in t_knn], knn_ms=knn_ms,
              project_ms=round(med(t_denoise) - sum(knn_ms.values()), 3), sigma=sigma, residual_rms_before=before,
              residual_rms_after=after, stats=info))
    if str(n) in args.host.split(","):
        ms, ref = host_mls(X.cpu().numpy())
        emit(dict(record="denoise_host_numpy", n=n, k=K, ms=round(ms, 1), max_abs_difference=float(np.abs(ref - out.cpu().numpy()).max())))
    del X, out
