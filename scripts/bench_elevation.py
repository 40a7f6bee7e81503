"""Time of the depth-to-elevation resampling (csrc/gbp_elev.h through geobipy_amd/elevation.py): 65 536 soundings x 440 depth cells onto
300 elevation cells (the mean over each cell) and onto 300 levels, and -- in the same process -- ``SibsonPlan.apply`` of the 300
resulting columns on the large synthetic survey of scripts/bench_survey_volume.py, which is the step a block of elevation columns feeds:

    python scripts/bench_elevation.py [--soundings 65536 --lines 64 --pixels 1000] [--depth-cells 440] [--cells 300] [--reps 20]
                                      [--out profiles/elevation/bench.json]

Device events around each call, two warm-up calls, medians; the two steps are timed in turn, twice.  The bytes are one read of the values
and one write of the output (what the algorithm needs; the surface and the axes are a few hundred KB).  Prints one line per measurement
and writes them as JSON to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geobipy_amd import _lib, elevation, gridding  # noqa: E402
from bench_survey_volume import medians, survey  # noqa: E402

HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--soundings", type=int, default=65536)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=1000)
    ap.add_argument("--depth-cells", type=int, default=440)
    ap.add_argument("--cells", type=int, default=300)
    ap.add_argument("--relief", type=float, default=40.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    x, y = survey(a.soundings, a.lines, a.pixels)
    N, n, E = x.size, a.depth_cells, a.cells
    rng = np.random.default_rng(3)
    d_edges = 0.5 * np.arange(n + 1)
    extent = x.max() - x.min()
    z = 100.0 + 0.5 * a.relief * (1.0 + np.sin(6.0 * (x - x.min()) / extent) * np.cos(4.0 * (y - y.min()) / extent)) + rng.uniform(-0.5, 0.5, N)
    edges = np.linspace(z.min() - d_edges[-1], z.max(), E + 1)
    levels = 0.5 * (edges[1:] + edges[:-1])
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    v = torch.randn((N, n), dtype=torch.float64, device=dev, generator=g)
    s = torch.as_tensor(z).to(dev)
    r = dict(soundings=N, depth_cells=n, elevation_cells=E, dz=float(edges[1] - edges[0]), relief=float(z.max() - z.min()), reps=a.reps,
             device=torch.cuda.get_device_name(0), bytes=N * (n + E) * 8)

    xe, ye = gridding.centred_mesh(x, y, 25.0, 25.0)
    plan = gridding.SibsonPlan(x, y, xe, ye, device=dev)
    r.update(nx=plan.nx, ny=plan.ny, list_total=plan.list_length)
    cols = elevation.resample(v, s, d_edges, edges=edges)
    r["finite_share"] = float(torch.isfinite(cols).double().mean())
    r["depth_cells_per_elevation_cell"] = float(edges[1] - edges[0]) / 0.5
    # the kernel alone: the C entry on arrays already on the device (``resample`` also checks and uploads the axes, on the host)
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    te, ted, tl, raw = torch.as_tensor(d_edges).to(dev), torch.as_tensor(edges).to(dev), torch.as_tensor(levels).to(dev), torch.empty_like(cols)

    def kernel(mode, axis):
        _lib.check(lib.gbp_elevation_resample(mode, N, 1, n, v.data_ptr(), s.data_ptr(), te.data_ptr(), E, axis.data_ptr(), 0, E,
                                              raw.data_ptr(), st))
    kernel(elevation.INTERVALS, ted)
    r["kernel_equals_resample"] = bool(torch.equal(torch.nan_to_num(raw, nan=-1e300), torch.nan_to_num(cols, nan=-1e300)))
    for turn in ("", "_again"):
        r["kernel_cells_ms" + turn] = medians(lambda: kernel(elevation.INTERVALS, ted), a.reps)[0]
        r["kernel_levels_ms" + turn] = medians(lambda: kernel(elevation.LEVELS, tl), a.reps)[0]
        r["resample_cells_ms" + turn], lo, hi = medians(lambda: elevation.resample(v, s, d_edges, edges=edges), a.reps)
        r["resample_cells_min_max_ms" + turn] = [lo, hi]
        r["resample_levels_ms" + turn] = medians(lambda: elevation.resample(v, s, d_edges, levels=levels), a.reps)[0]
        r["apply_ms" + turn], lo, hi = medians(lambda: plan.apply(cols), max(3, a.reps // 2))
        r["apply_min_max_ms" + turn] = [lo, hi]
    for k in ("cells", "levels"):
        ms = max(r["kernel_%s_ms" % k], r["kernel_%s_ms_again" % k])
        r["kernel_%s_TBps" % k] = r["bytes"] / ms / 1e9
        r["kernel_%s_share_of_hbm" % k] = r["bytes"] / ms / 1e9 / HBM_TBPS
    r["resample_over_apply"] = max(r["resample_cells_ms"], r["resample_cells_ms_again"]) / min(r["apply_ms"], r["apply_ms_again"])
    r["resample_costs_less_than_apply"] = bool(r["resample_over_apply"] < 1.0)
    # thick cells, for the sum's other branches: 30 cells of ~17 depth cells, 3 of ~170
    for cells in (30, 3):
        ek = np.linspace(edges[0], edges[-1], cells + 1)
        r["resample_%d_cells_ms" % cells] = medians(lambda: elevation.resample(v, s, d_edges, edges=ek), a.reps)[0]
    for k, val in r.items():
        print("%s: %s" % (k, ("%.4g" % val) if isinstance(val, float) else val))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
