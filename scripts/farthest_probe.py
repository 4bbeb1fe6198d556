"""Times of farthest point sampling (records under profiles/farthest/).

    python scripts/farthest_probe.py [--n 256,...,10000000] [--m 1024] [--runs 7] [--out FILE]

One JSON line per size of --n; --out appends them to a file.  The cloud is a float64 device tensor, uniform in a 20 m cube; the
picks and distances leave into device memory.  Two contexts: one with SICP_FARTHEST_ONE_MAX at its limit (the single workgroup up
to 12 288 rows), one with 0 (always the stepped path).  Per size, after a warm-up call of each, --runs runs of
  one        sicp_farthest on the single-workgroup path (n <= 12 288), the whole call
  stepped    sicp_farthest on the stepped path, the whole call: m + 2 launches, enqueued blind
  torch      the same sequence in torch float64: per pick torch.minimum of m_i with the squared distances to the last pick
             (the difference tensor materialised) and argmax, the pick kept on the device
  read       X.sum(): one pass over the cloud, repeated -- a cloud of up to 10 M rows (240 MB) fits the last-level cache
  read_big   the same sum over a 1 GiB tensor, four times the last-level cache: the streaming rate from memory, which the
             stepped path is held against
as wall times between device synchronisations: median, minimum and maximum.  `same_picks`: both paths and torch agree on the
picks (torch's rounding is not the contract's and its argmax has no tie rule: a uniform cloud has no ties to break).

    timeout -k 10 500 python scripts/farthest_probe.py --out profiles/farthest/probe.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simpleicp_amd import _lib
from simpleicp_amd.tensors import _wait_for_torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="256,1024,2048,4096,6144,8192,10240,12288,16384,32768,100000,1000000,10000000")
ap.add_argument("--m", type=int, default=1024)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
DEV = "cuda:0"


def context(one_max):
    old = os.environ.get("SICP_FARTHEST_ONE_MAX")
    os.environ["SICP_FARTHEST_ONE_MAX"] = str(one_max)
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ["SICP_FARTHEST_ONE_MAX"]
        else:
            os.environ["SICP_FARTHEST_ONE_MAX"] = old


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def series(fn, runs):
    timed(fn)
    t = [timed(fn)[0] for _ in range(runs)]
    return dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))


one, stepped = context(_lib.FARTHEST_ONE_LIMIT), context(0)
BIG = torch.rand(1 << 27, dtype=torch.float64, device=DEV)
READ_BIG = series(lambda: BIG.sum(), args.runs)
for n in (int(v) for v in args.n.split(",") if v):
    m = min(args.m, n)
    X = torch.rand((n, 3), dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(n)) * 20.0 - 10.0
    idx = {k: torch.empty(m, dtype=torch.int64, device=DEV) for k in ("one", "stepped")}
    d2 = torch.empty(m, dtype=torch.float64, device=DEV)
    rec = dict(record="farthest_cost", n=n, m=m, runs=args.runs)

    def run(ctx, name):
        return ctx.farthest(X.data_ptr(), m, n=n, idx_ptr=idx[name].data_ptr(), d2_ptr=d2.data_ptr())

    for name, ctx in (("one", one), ("stepped", stepped)):
        if name == "one" and n > _lib.FARTHEST_ONE_LIMIT:
            continue
        _wait_for_torch(ctx, X.device)
        rec["stats"] = run(ctx, name).as_dict()
        rec[name + "_ms"] = series(lambda: run(ctx, name), args.runs)
    rec["stepped_us_per_pick"] = round(rec["stepped_ms"]["median"] * 1e3 / m, 3)

    def in_torch():
        mi = torch.full((n,), float("inf"), dtype=torch.float64, device=DEV)
        s = torch.zeros(1, dtype=torch.int64, device=DEV)
        picks = torch.empty(m, dtype=torch.int64, device=DEV)
        for t in range(m):
            picks[t] = s[0]
            mi = torch.minimum(mi, ((X - X.index_select(0, s)) ** 2).sum(1))
            s = torch.argmax(mi).view(1)
        return picks

    rec["torch_ms"] = series(in_torch, args.runs)
    picks = in_torch()
    rec["same_picks"] = bool(torch.equal(picks, idx["stepped"]) and (n > _lib.FARTHEST_ONE_LIMIT or torch.equal(picks, idx["one"])))
    rec["read_ms"] = series(lambda: X.sum(), args.runs)
    rec["read_GBps"] = round(24.0 * n / (rec["read_ms"]["median"] * 1e-3) / 1e9, 1)
    rate = BIG.numel() * 8.0 / (READ_BIG["median"] * 1e-3)
    rec["read_big_ms"], rec["read_big_GBps"] = READ_BIG, round(rate / 1e9, 1)
    # a pick reads every m_i (8 n bytes) and every row (24 n) and writes the m_i that fell (at most 8 n)
    rec["bound_us_per_pick_32n"] = round(32.0 * n / rate * 1e6, 3)
    rec["bound_us_per_pick_40n"] = round(40.0 * n / rate * 1e6, 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del X
one.close()
stepped.close()
