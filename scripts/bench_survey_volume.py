"""Time of the survey-volume gridding (csrc/gbp_grid.h through geobipy_amd/gridding.py) on a synthetic survey of jittered flight lines:
the plan (once per grid) and ``apply`` on [N, columns] (the hot path), against the same cover lists applied by torch on the device in
the same process -- a ``torch.sparse_csr`` product and a chunked ``index_add_``, neither of which keeps the order of the sums --
and, for scale on the small survey only, the numpy / torch statement of the algorithm on the CPU (tests/sibson_reference.py):

    python scripts/bench_survey_volume.py [--soundings 65536 --lines 64 --pixels 1000] [--columns 440] [--reps 10]
                                          [--cpu] [--out profiles/survey_volume/bench.json]

Device events around each call, two warm-up calls, medians.  Prints one line per measurement and writes them as JSON to --out."""
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
from geobipy_amd import gridding  # noqa: E402


def survey(n_soundings, n_lines, pixels, spacing=25.0, seed=1):
    """Soundings of ``n_lines`` flight lines along x, jittered, over ~pixels x pixels cells of ``spacing`` metres."""
    rng = np.random.default_rng(seed)
    per = n_soundings // n_lines
    extent = (pixels - 1.5) * spacing
    x = np.tile(np.linspace(0.0, extent, per), n_lines) + rng.uniform(-0.3, 0.3, per * n_lines) * extent / per
    y = np.repeat(np.linspace(0.0, extent, n_lines), per) + rng.uniform(-0.08, 0.08, per * n_lines) * extent / n_lines
    x[0], x[-1], y[0], y[-1] = 0.0, extent, 0.0, extent                     # pin the bounding box
    return 400000.0 + np.clip(x, 0.0, extent), 6200000.0 + np.clip(y, 0.0, extent)


def medians(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def cover_pairs(D):
    """(dest, src) flat pixel numbers of every covering pair, sorted by dest, built by torch on the device from D [ny, nx]."""
    ny, nx = D.shape
    dev = D.device
    dests, srcs = [], []
    for d in torch.unique(D).tolist():
        if d == 0:
            continue
        w = min(d, nx + ny)
        si, sj = torch.nonzero(D == d, as_tuple=True)
        o = torch.arange(-w, w, device=dev)
        oi, oj = torch.meshgrid(o, o, indexing="ij")
        keep = (oi * oi + oj * oj) <= d * d
        oi, oj = oi[keep], oj[keep]
        step = max(1, (1 << 26) // max(1, oi.numel()))
        for a in range(0, si.numel(), step):
            ti = si[a:a + step, None] + oi[None, :]
            tj = sj[a:a + step, None] + oj[None, :]
            ok = (ti >= 0) & (ti < ny) & (tj >= 0) & (tj < nx)
            dests.append((ti * nx + tj)[ok])
            srcs.append((si[a:a + step] * nx + sj[a:a + step])[:, None].expand_as(ti)[ok])
    dest, src = torch.cat(dests), torch.cat(srcs)
    order = torch.argsort(dest)
    return dest[order], src[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--soundings", type=int, default=65536)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=1000)
    ap.add_argument("--columns", type=int, default=440)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--plan-reps", type=int, default=10)
    ap.add_argument("--yardstick-reps", type=int, default=10)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="also time the numpy / torch formulation on the CPU (small surveys only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    x, y = survey(a.soundings, a.lines, a.pixels)
    xe, ye = gridding.centred_mesh(x, y, 25.0, 25.0)
    N, C, nx, ny = x.size, a.columns, xe.size - 1, ye.size - 1
    P = nx * ny
    r = dict(soundings=N, lines=a.lines, nx=nx, ny=ny, columns=C, reps=a.reps, device=torch.cuda.get_device_name(0))

    # the plan: a host clock around the call (it ends in a synchronise: the scan of n is the host's)
    ts = []
    plan = None
    for _ in range(a.plan_reps + 1):
        if plan is not None:
            plan.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = gridding.SibsonPlan(x, y, xe, ye, device=dev)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    n = plan.count.flatten().to(torch.int64)
    r.update(plan_ms=float(np.median(ts[1:])), plan_first_ms=ts[0], list_total=plan.list_length, list_longest=plan.longest_list,
             list_median=int(n.median()), list_mean=plan.list_length / P, plan_bands=plan.n_bands, plan_bytes=plan.bytes_held,
             uncovered_pixels=int((n == 0).sum()), D_max=int(plan.distance.max()))

    g = torch.Generator(device=dev)
    g.manual_seed(2)
    v = torch.randn((N, C), dtype=torch.float64, device=dev, generator=g)
    out = plan.apply(v)
    med, lo, hi = medians(lambda: plan.apply(v), a.reps)
    list_bytes = plan.list_length * (C * 8 + 4)
    out_bytes = P * C * 8
    r.update(apply_ms=med, apply_min_ms=lo, apply_max_ms=hi, apply_ms_per_column=med / C,
             list_read_TBps=(list_bytes + out_bytes) / med / 1e9, floor_bytes=N * C * 8 + out_bytes,
             floor_TBps=(N * C * 8 + out_bytes) / med / 1e9, values_MB=N * C * 8 / 1e6, output_GB=out_bytes / 1e9)
    for cols in (1, 64):
        if cols < C:
            vc = v[:, :cols].contiguous()
            r["apply_%d_columns_ms" % cols] = medians(lambda: plan.apply(vc), a.reps)[0]
    r["plan_over_apply"] = r["plan_ms"] / med

    if not a.no_yardstick:
        dest, src = cover_pairs(plan.distance.to(torch.int64))
        assert dest.numel() == plan.list_length and bool(torch.equal(torch.bincount(dest, minlength=P), n))
        who = plan.index.flatten().to(torch.int64)[src]
        del src
        crow = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        crow[1:] = torch.cumsum(n, 0)
        nf = n.to(torch.float64)[:, None]
        A = torch.sparse_csr_tensor(crow, who, torch.ones(who.numel(), dtype=torch.float64, device=dev), size=(P, N))
        spmm = lambda: (A @ v) / nf                                             # noqa: E731  ([P, C]: no transpose, no mask)
        got = spmm()
        fin = ~torch.isnan(out[0].flatten())
        r["yardstick_max_abs_diff"] = float((got.T.reshape(C, ny, nx)[:, fin.reshape(ny, nx)] - out[:, fin.reshape(ny, nx)]).abs().max())
        del got
        r["sparse_csr_ms"] = medians(spmm, a.yardstick_reps)[0]
        acc = torch.empty((P, C), dtype=torch.float64, device=dev)
        chunk = max(1, (1 << 30) // (C * 8))                                    # 1 GiB of gathered rows at a time

        def index_add():
            acc.zero_()
            for p0 in range(0, who.numel(), chunk):
                acc.index_add_(0, dest[p0:p0 + chunk], v[who[p0:p0 + chunk]])
            return acc.div_(nf)
        r["index_add_ms"] = medians(index_add, max(3, a.yardstick_reps // 3), warm=1)[0]
        # the hand-written gather again, after the yardsticks: both medians from the same process
        r["apply_again_ms"] = medians(lambda: plan.apply(v), a.reps)[0]
        best = min(r["sparse_csr_ms"], r["index_add_ms"])
        r["yardstick"] = "sparse_csr" if best == r["sparse_csr_ms"] else "index_add"
        r["yardstick_over_apply"] = best / max(r["apply_ms"], r["apply_again_ms"])

    if a.cpu:
        import sibson_reference as sr
        vh = v[:, :1].cpu().numpy()
        t0 = time.perf_counter()
        px, py, dx, dy = sr.pixel_coordinates(x, y, xe, ye)
        index, D = sr.nearest(px, py, nx, ny)
        t1 = time.perf_counter()
        dd, ss = sr.cover(D)
        t2 = time.perf_counter()
        ref = sr.apply(vh, index, D, dd, ss)
        t3 = time.perf_counter()
        r.update(cpu_nearest_s=t1 - t0, cpu_cover_s=t2 - t1, cpu_apply_one_column_s=t3 - t2, cpu_threads=torch.get_num_threads(),
                 cpu_equals_device=bool(np.array_equal(ref[0], out[0].cpu().numpy(), equal_nan=True)))
    for k, val in r.items():
        print("%s: %s" % (k, ("%.4g" % val) if isinstance(val, float) else val))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
