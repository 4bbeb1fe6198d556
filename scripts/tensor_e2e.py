"""End to end: run_tensors (clouds as torch tensors on the GPU) against SimpleICP.run (clouds on the host), and run_batch with device
pairs against host pairs.  Every timing is a host clock around a call that returns complete (both roads end in a device
synchronise), after warm-up, repeated; the outputs are checked against run() on the same seeded clouds.

    python scripts/tensor_e2e.py --out profiles/tensors/e2e.jsonl          # C4: 10 M vs 10 M, Q = 1000; batch: 64 x 100 k
    python scripts/tensor_e2e.py --only c4 --tensors-only --repeats 1 --warmup 1    # the case a rocprofv3 trace is taken of
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def surface_pair(n, seed, shift=(0.3, -0.2, 0.1), yaw=0.02):
    rng = np.random.default_rng(seed)
    half = np.sqrt(n / 10.0) / 2
    xy = rng.uniform(-half, half, (n, 2))
    z = 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, n)
    Xf = np.column_stack((xy, z))
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (Xf + rng.normal(0, 0.005, Xf.shape)) @ R.T + np.array(shift)
    return Xf, Xm


def surface_pair_on_device(n, seed, dev, shift=(0.3, -0.2, 0.1), yaw=0.02):
    """The same kind of pair made on the device with torch's generator (--tensors-only: no input crosses the link either)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    half = float(np.sqrt(n / 10.0) / 2)
    xy = (torch.rand((n, 2), generator=g, device=dev, dtype=torch.float64) * 2 - 1) * half
    z = 2 * torch.sin(xy[:, 0] / 4) * torch.cos(xy[:, 1] / 6) + 0.005 * torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    Xf = torch.stack((xy[:, 0], xy[:, 1], z), 1)
    c, s = float(np.cos(yaw)), float(np.sin(yaw))
    R = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64, device=dev)
    Xm = (Xf + 0.005 * torch.randn(Xf.shape, generator=g, device=dev, dtype=torch.float64)) @ R.T
    return Xf, Xm + torch.tensor(shift, dtype=torch.float64, device=dev)


def timed(fn, warmup, repeats, setup=None):
    """The clock brackets fn alone, the way bench.end_to_end times run(): setup() (the DataFrames, the SimpleICP object) runs before
    it and its value is fn's argument; fn's result and that argument are held until the clock has stopped and are dropped after it
    (freeing a 240 MB transformed cloud or a frame is the caller's munmap, not the registration's).  Returns the last result and the
    times of the repeats in ms."""
    import torch
    out, ts = None, []
    for i in range(warmup + repeats):
        arg = setup() if setup is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        held = fn(arg) if setup is not None else fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        out = held                                     # (the previous result is dropped here, outside the clock)
        del held, arg
        if i >= warmup:
            ts.append(dt)
    return out, ts


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "repeats": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--q", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--pair-n", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=["c4", "batch"], default=None)
    ap.add_argument("--tensors-only", action="store_true", help="C4: run_tensors only, no run() and no comparison (a copy trace "
                    "then lists what run_tensors moves, nothing else)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from simpleicp_amd import PointCloud, SimpleICP, run_batch, run_tensors
    dev = torch.device("cuda", 0)
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    if a.only in (None, "c4"):
        Xf, Xm = surface_pair_on_device(a.n, 0, dev) if a.tensors_only else surface_pair(a.n, 0)
        kw = dict(correspondences=a.q)

        def frames():
            icp = SimpleICP(verbose=False)
            # (a 2-D array goes into the frame without a copy; run() replaces the movable frame's columns, the array stays as it is)
            icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]))
            return icp
        if not a.tensors_only:
            ref, t_host = timed(lambda icp: icp.run(**kw), a.warmup, a.repeats, setup=frames)
            emit({"case": "c4_run_host", "n": a.n, "q": a.q, **stats(t_host)})
        for dtype in (torch.float64, torch.float32):
            tf, tm = ((Xf.to(dtype), Xm.to(dtype)) if a.tensors_only
                      else (torch.tensor(Xf, dtype=dtype, device=dev), torch.tensor(Xm, dtype=dtype, device=dev)))
            res, t_dev = timed(lambda: run_tensors(tf, tm, **kw), a.warmup, a.repeats)
            if a.tensors_only:
                same = None
            elif dtype == torch.float64:
                same = (np.array_equal(res.H, ref[0]) and np.array_equal(res.residuals, ref[3])
                        and np.array_equal(res.X_mov_transformed.cpu().numpy(), ref[1]))
            else:                                           # (against run() on the widened float32 clouds)
                icp = SimpleICP(verbose=False)
                icp.add_point_clouds(PointCloud(tf.double().cpu().numpy(), columns=["x", "y", "z"]),
                                     PointCloud(tm.double().cpu().numpy(), columns=["x", "y", "z"]))
                r32 = icp.run(**kw)
                same = (np.array_equal(res.H, r32[0]) and np.array_equal(res.residuals, r32[3])
                        and np.array_equal(res.X_mov_transformed.cpu().numpy(), r32[1].astype(np.float32)))
            emit({"case": f"c4_run_tensors_{str(dtype).split('.')[-1]}", "n": a.n, "q": a.q, "equal_to_run": same if same is None else bool(same),
                  "iterations": res.iterations, **stats(t_dev)})
            del tf, tm, res

    if a.only in (None, "batch"):
        host_pairs = [surface_pair(a.pair_n, 100 + i) for i in range(a.pairs)]
        dev_pairs = [(torch.tensor(f, device=dev), torch.tensor(m, device=dev)) for f, m in host_pairs]
        out_h, t_h = timed(lambda: run_batch(host_pairs, correspondences=a.q), a.warmup, a.repeats)
        out_d, t_d = timed(lambda: run_batch(dev_pairs, correspondences=a.q), a.warmup, a.repeats)
        same = all(np.array_equal(h.H, d.H) and np.array_equal(h.residuals, d.residuals)
                   and np.array_equal(h.X_mov_transformed, d.X_mov_transformed.cpu().numpy()) for h, d in zip(out_h, out_d))
        emit({"case": "batch_host_pairs", "pairs": a.pairs, "n": a.pair_n, "q": a.q, **stats(t_h)})
        emit({"case": "batch_device_pairs", "pairs": a.pairs, "n": a.pair_n, "q": a.q, "equal_to_host_pairs": bool(same), **stats(t_d)})

    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
