"""Time of the line-products kernel (csrc/gbp_hitmap.h k_hitmap_products) on one line of synthetic layered hit maps, against its HBM bytes,
k_hitmap_stats on the same block and the torch formulation on 16 CPU threads:

    python scripts/bench_line_products.py [--B 8192] [--reps 20] [--cpu-B 128] [--out profiles/line_products/bench.json]

Prints one line per measurement and writes them as JSON to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_products_reference  # noqa: E402
from geobipy_amd import hitmap, line_products  # noqa: E402

HBM_TBS = 6.3                                   # achievable HBM read bandwidth of an MI355X, TB/s (the guide's figure, not measured here)


def layered_maps(B, nv, nz, dev, seed=1):
    """B hit maps [B, nv, nz] like the chains leave: 40 (value cell, depth range) bars of random height per sounding."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    hm = torch.zeros((B, nv, nz), dtype=torch.int32, device=dev)
    z = torch.arange(nz, device=dev)[None, :]
    rows = torch.arange(B, device=dev)
    for _ in range(40):
        v = torch.randint(0, nv, (B,), device=dev, generator=g)
        lo = torch.randint(0, nz, (B,), device=dev, generator=g)
        hi = torch.clamp(lo + torch.randint(1, 200, (B,), device=dev, generator=g), max=nz)
        bar = ((z >= lo[:, None]) & (z < hi[:, None])).to(torch.int32) * torch.randint(1, 300, (B, 1), device=dev, generator=g, dtype=torch.int32)
        hm[rows, v] += bar
    return hm


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-B", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nv, nz = 250, 440
    dev = torch.device("cuda", 0)
    hm = layered_maps(a.B, nv, nz, dev)
    lmp = torch.zeros(a.B, dtype=torch.float64, device=dev)
    q, _, _ = line_products.quantiles()
    depth_edges = np.arange(nz + 1) * 0.5
    map_bytes = a.B * nv * nz * 4
    out_bytes = a.B * nz * (8 + 4 + 8 + 8 + 4 * len(q))             # mean, mode_idx, total, s1, q_idx
    r = dict(B=a.B, n_value=nv, n_depth=nz, n_quantiles=len(q), map_bytes=map_bytes, reps=a.reps)
    r["products_kernel_ms"] = timed(lambda: hitmap.moments(hm, lmp, 2.3, q), a.reps)
    r["statistics_kernel_ms"] = timed(lambda: hitmap.statistics(hm, lmp, 2.3), a.reps)
    r["products_with_finishing_ms"] = timed(lambda: hitmap.products(hm, lmp, 2.3, depth_edges=depth_edges), a.reps)
    r["products_GBps"] = (map_bytes + out_bytes) / r["products_kernel_ms"] / 1e6
    r["products_fraction_of_hbm"] = r["products_GBps"] / (HBM_TBS * 1e3)
    r["statistics_GBps"] = (map_bytes + 4 * a.B * nz * 8) / r["statistics_kernel_ms"] / 1e6
    r["products_over_statistics"] = r["products_kernel_ms"] / r["statistics_kernel_ms"]

    # the kernel against the torch formulation on a slice (a check of what was timed)
    s = slice(0, 64)
    m = hitmap.moments(hm[s], lmp[s], 2.3, q)
    t = line_products_reference.moments_torch(hm[s], lmp[s], 2.3, q)
    r["check_integer_outputs_equal"] = bool(torch.equal(m["q_idx"], t["q_idx"]) and torch.equal(m["mode_idx"], t["mode_idx"])
                                            and torch.equal(m["total"], t["total"]))
    r["check_s1_max_rel"] = float(((m["s1"] - t["s1"]).abs() / t["s1"].abs().clamp(min=1e-300)).max())

    # upload of one 4 096-sounding block from pageable host memory (what from_results does per block)
    host = hm[:4096].cpu()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host.to(dev)
    torch.cuda.synchronize()
    r["upload_4096_ms"] = (time.perf_counter() - t0) * 1e3
    r["upload_GBps"] = host.numel() * 4 / r["upload_4096_ms"] / 1e6

    # the torch formulation of the same moments on 16 CPU threads, at cpu-B soundings, scaled to B
    torch.set_num_threads(16)
    hc, lc = hm[:a.cpu_B].cpu(), lmp[:a.cpu_B].cpu()
    line_products_reference.moments_torch(hc[:4], lc[:4], 2.3, q)
    t0 = time.perf_counter()
    line_products_reference.moments_torch(hc, lc, 2.3, q)
    r["cpu_torch_16_threads_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * a.B / a.cpu_B
    r["cpu_B"] = a.cpu_B
    r["device"] = torch.cuda.get_device_name(0)
    for k, v in r.items():
        print("%s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
