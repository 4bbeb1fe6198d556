"""Summarises the csv output of `rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -o c4 -- python
scripts/tensor_e2e.py --only c4 --tensors-only --repeats 1 --warmup 1`: the ingest / egress kernels' achieved bytes/s against HBM,
what went over the copy engines, and the runtime's small blit copies.

    python scripts/tensor_trace_summary.py DIR --n 10000000 --out profiles/tensors/c4_trace_summary.json

Bytes per point are what the kernels must move: k_ingest reads 3 coordinates of the input dtype and writes 3 float64 columns;
k_egress reads 3 float64 columns and writes 3 values of the output dtype.  HBM: 8.0 TB/s spec, ~6.3 TB/s achievable (float4 copy).
"""
import argparse
import csv
import json
from pathlib import Path

HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    d = Path(a.dir)
    kernels = list(csv.DictReader(open(next(d.glob("*kernel_stats.csv")))))
    rates = []
    for k in kernels:
        name = k["Name"]
        if "k_ingest" not in name and "k_egress" not in name:
            continue
        size = 8 if ("<double" in name) else 4
        b = a.n * 3 * (size + 8)
        t = float(k["AverageNs"]) / 1e9
        rates.append({"kernel": name.split(">(")[0] + ">", "calls": int(k["Calls"]), "average_us": t * 1e6, "bytes": b, "bytes_per_s": b / t,
                       "of_hbm_spec": b / t / HBM_SPEC, "of_hbm_achievable": b / t / HBM_ACHIEVABLE})
    blits = [k for k in kernels if k["Name"].startswith("__amd_rocclr_copyBuffer")]
    copies = list(d.glob("*memory_copy_stats.csv"))
    summary = {
        "n": a.n,
        "streaming_kernels": rates,
        # DMA copies the memory-copy trace recorded (none: no memory_copy_stats file is written when there are none)
        "memory_copies": [dict(r) for r in csv.DictReader(open(copies[0]))] if copies else [],
        # small copies the runtime runs as blit kernels (statistics words, the Q picked positions, normals into the ctx)
        "blit_copies": {"calls": int(blits[0]["Calls"]), "max_us": float(blits[0]["MaxNs"]) / 1e3} if blits else None,
    }
    Path(a.out).write_text(json.dumps(summary, indent=1) + "\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
