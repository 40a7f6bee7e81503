"""Time of the pixel-posterior pool (csrc/gbp_grid.h k_sibson_pool) on the small survey of bench_survey_volume.py -- 8 192 soundings in
32 lines on 249 x 249 pixels -- with synthetic layered hit maps of 250 x 440 and one block of 2 048 pixels from the middle of the raster:

    python scripts/bench_pixel_posteriors.py [--soundings 8192 --lines 32 --pixels 250] [--block 2048] [--reps 10]
                                             [--out profiles/pixel_posteriors/bench.json]

  (a) k_sibson_pool with and without the axis offsets u;
  (b) the torch formulation of the same sum over the same lists (no offsets): ``index_add_`` of gathered maps, chunked to 1 GiB;
  (c) ``SibsonPlan.apply``, the closest existing kernel, on a few value rows of the same maps as float64 columns over the whole raster
      (it cannot take a block of pixels): compared per (pixel, cell), it reads twice the bytes and writes transposed.  No bar.

Every candidate runs on preallocated buffers, (a) through the C entry, and is timed with device events, one launch per event pair, the
candidates alternating inside each repetition of one process; medians after a warm-up.  The bar: (a) is faster than (b).  Bytes over
time are given by two counts: one read of the maps the block touches plus the write, and the reads of every list entry plus the write.
Prints one line per measurement and writes them as JSON to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_intervals import alternating  # noqa: E402
from bench_line_products import layered_maps  # noqa: E402
from bench_survey_volume import cover_pairs, survey  # noqa: E402
from geobipy_amd import _lib, gridding, line_products  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--soundings", type=int, default=8192)
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--pixels", type=int, default=250)
    ap.add_argument("--block", type=int, default=2048)
    ap.add_argument("--apply-rows", type=int, default=4, help="value rows of the maps that (c) grids as float64 columns")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nv, nz, hw = 250, 440, 2.3
    x, y = survey(a.soundings, a.lines, a.pixels)
    xe, ye = gridding.centred_mesh(x, y, 25.0, 25.0)
    plan = gridding.SibsonPlan(x, y, xe, ye, device=dev)
    N, nx, ny = x.size, plan.nx, plan.ny
    P, B = nx * ny, min(a.block, nx * ny)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    maps = layered_maps(N, nv, nz, dev)
    max_total = int(maps.sum(dim=1, dtype=torch.int64).max())
    rng = np.random.default_rng(4)
    lmp = (-2.0 + rng.normal(0.0, 0.1, N)) * line_products.LN10            # prior means a few value cells apart
    u = torch.as_tensor(gridding.axis_offsets(lmp, hw, nv)).to(dev)
    p0 = min(max(0, (ny // 2) * nx - B // 2), P - B)
    pixels = torch.arange(p0, p0 + B, dtype=torch.int32, device=dev)
    pooled = torch.empty((B, nv, nz), dtype=torch.int32, device=dev)
    clipped = torch.empty((B, nz), dtype=torch.int64, device=dev)
    r = dict(soundings=N, lines=a.lines, nx=nx, ny=ny, n_value=nv, n_depth=nz, block=B, first_pixel=p0, reps=a.reps,
             list_longest=plan.longest_list, device=torch.cuda.get_device_name(0))

    def pool(offsets):
        _lib.check(lib.gbp_sibson_pool(plan._handle, B, pixels.data_ptr(), nv, nz, maps.data_ptr(), offsets, max_total, pooled.data_ptr(),
                                       clipped.data_ptr(), stream))

    # (b): the block's list entries as (row of the block, sounding) pairs, from the plan's geometry by torch
    dest, src = cover_pairs(plan.distance.to(torch.int64))
    keep = (dest >= p0) & (dest < p0 + B)
    row, who = (dest[keep] - p0), plan.index.flatten().to(torch.int64)[src[keep]]
    del dest, src, keep
    E = int(who.numel())
    touched = int(torch.unique(who).numel())
    flat = maps.view(N, nv * nz)
    acc = torch.empty((B, nv * nz), dtype=torch.int32, device=dev)
    chunk = max(1, (1 << 30) // (nv * nz * 4))

    def index_add():
        acc.zero_()
        for e0 in range(0, E, chunk):
            acc.index_add_(0, row[e0:e0 + chunk], flat[who[e0:e0 + chunk]])

    # (c): a few value rows as float64 columns through the gather, the whole raster
    rows = min(a.apply_rows, nv)
    cols = maps[:, nv // 2:nv // 2 + rows, :].reshape(N, rows * nz).to(torch.float64).contiguous()
    grid = torch.empty((rows * nz, ny, nx), dtype=torch.float64, device=dev)

    def apply():
        _lib.check(lib.gbp_sibson_apply(plan._handle, rows * nz, cols.data_ptr(), grid.data_ptr(), stream))

    t = alternating({"pool": lambda: pool(None), "pool_offsets": lambda: pool(u.data_ptr()), "index_add": index_add, "apply": apply}, a.reps)
    for k, ms in t.items():
        r[k + "_ms"] = ms
    pool(None)
    index_add()
    torch.cuda.synchronize()
    r["pool_equals_index_add"] = bool(torch.equal(pooled.view(B, nv * nz), acc))
    pool(u.data_ptr())
    torch.cuda.synchronize()
    r["clipped_share_of_block"] = float(clipped.sum()) / max(1.0, float(clipped.sum() + pooled.sum(dtype=torch.int64)))
    out_bytes = B * nv * nz * 4 + B * nz * 8
    r.update(list_entries=E, list_mean=E / B, soundings_touched=touched, once_bytes=touched * nv * nz * 4 + out_bytes,
             list_bytes=E * (nv * nz * 4 + 4) + out_bytes)
    for k in ("pool", "pool_offsets"):
        r[k + "_once_TBps"] = r["once_bytes"] / t[k] / 1e9
        r[k + "_list_TBps"] = r["list_bytes"] / t[k] / 1e9
    r["index_add_over_pool"] = t["index_add"] / t["pool"]
    r["pool_meets_the_bar"] = bool(t["pool"] < t["index_add"] and r["pool_equals_index_add"])
    # per (pixel, cell): the pool's block against the gather's raster
    r["pool_ns_per_pixel_cell"] = t["pool"] * 1e6 / (B * nv * nz)
    r["apply_ns_per_pixel_cell"] = t["apply"] * 1e6 / (P * rows * nz)
    r["apply_over_pool_per_pixel_cell"] = r["apply_ns_per_pixel_cell"] / r["pool_ns_per_pixel_cell"]
    for k, v in r.items():
        print("%s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    plan.close()


if __name__ == "__main__":
    main()
