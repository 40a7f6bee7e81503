"""Time of the interval-marginal kernel (csrc/gbp_hitmap.h k_hitmap_intervals) on one line of synthetic layered hit maps -- a shared
partition of 8 intervals, and per-sounding ranges with M = 40 -- against k_hitmap_classes at K = 1 (the project's fastest single read
of the same maps) and the torch formulation (an int64 cumulative sum along depth and two gathers), and of the 64-bit products /
classes kernels on the marginals:

    python scripts/bench_intervals.py [--B 8192] [--reps 20] [--out profiles/intervals/bench.json]

Every kernel is launched through its C entry on preallocated buffers and timed with device events, one launch per event pair, the
candidates alternating inside each repetition of one process; the figures are medians after a warm-up.  Prints one line per
measurement and writes them as JSON to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_line_products import HBM_TBS, layered_maps  # noqa: E402
from geobipy_amd import _lib, hitmap, intervals, line_products  # noqa: E402


def marginals_torch(hm, lo, hi):
    """The torch formulation: an int64 prefix along depth and two gathers (ranges [B, M] inside [0, n_depth], lo <= hi)."""
    B, nv, nz = hm.shape
    P = torch.zeros((B, nv, nz + 1), dtype=torch.int64, device=hm.device)
    P[:, :, 1:] = torch.cumsum(hm, dim=2, dtype=torch.int64)
    g = lambda i: torch.gather(P, 2, i.long()[:, None, :].expand(B, nv, i.shape[1]))       # noqa: E731
    return g(hi) - g(lo)


def alternating(fns, reps, warmup=3):
    """{name: median ms} of the launches ``fns`` ({name: callable}), each timed by its own pair of device events, the candidates
    taking turns inside every repetition."""
    times = {k: [] for k in fns}
    for rep in range(warmup + reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, nv, nz, hw = a.B, 250, 440, 2.3
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    hm = layered_maps(B, nv, nz, dev)
    lmp = torch.full((B,), -2.0 * line_products.LN10, dtype=torch.float64, device=dev)
    depth_edges = np.arange(nz + 1) * 0.5
    map_bytes = B * nv * nz * 4
    r = dict(B=B, n_value=nv, n_depth=nz, map_bytes=map_bytes, reps=a.reps)

    # the ranges: one partition of 8 for every sounding; 40 elevation intervals under a different surface per sounding
    shared = intervals.depth_ranges(depth_edges, [0.0, 5.0, 10.0, 20.0, 30.0, 50.0, 75.0, 120.0, 220.0])
    surface = np.random.default_rng(4).uniform(80.0, 140.0, B)
    own = intervals.elevation_ranges(surface, depth_edges, np.arange(-100.0, 141.0, 6.0))
    sets = {}
    for name, rr in (("shared_8", shared), ("per_sounding_40", own)):
        lo = torch.as_tensor(np.broadcast_to(rr.lo, (B, rr.lo.shape[-1])).copy()).to(dev)
        hi = torch.as_tensor(np.broadcast_to(rr.hi, (B, rr.hi.shape[-1])).copy()).to(dev)
        sets[name] = (lo, hi, torch.empty((B, nv, lo.shape[1]), dtype=torch.int64, device=dev))
    assert sets["shared_8"][0].shape[1] == 8 and sets["per_sounding_40"][0].shape[1] == 40

    def interval_kernel(name):
        lo, hi, out = sets[name]
        return lambda: _lib.check(lib.gbp_hitmap_intervals(B, nv, nz, lo.shape[1], hm.data_ptr(), lo.data_ptr(), hi.data_ptr(), out.data_ptr(), stream))

    mu, sd = (ctypes.c_double * 1)(-2.0), (ctypes.c_double * 1)(0.4)
    prob = torch.empty((B, 1, nz), dtype=torch.float64, device=dev)
    best = torch.empty((B, nz), dtype=torch.int32, device=dev)
    best_p = torch.empty((B, nz), dtype=torch.float64, device=dev)

    def classes_1():
        _lib.check(lib.gbp_hitmap_classes(B, nv, nz, hm.data_ptr(), lmp.data_ptr(), hw, 1, mu, sd, prob.data_ptr(), best.data_ptr(), best_p.data_ptr(),
                                          stream))

    def torch_formulation(name):
        lo, hi, _ = sets[name]
        return lambda: marginals_torch(hm, lo, hi)

    t = alternating({"intervals_shared_8": interval_kernel("shared_8"), "classes_1": classes_1,
                     "intervals_per_sounding_40": interval_kernel("per_sounding_40")}, a.reps)
    t.update(alternating({"torch_shared_8": torch_formulation("shared_8"), "torch_per_sounding_40": torch_formulation("per_sounding_40")},
                         max(3, a.reps // 4), warmup=1))
    for k, ms in t.items():
        r[k + "_ms"] = ms
    for name in sets:
        M = sets[name][0].shape[1]
        ms = t["intervals_" + name]
        nbytes = map_bytes + B * nv * M * 8 + 2 * B * M * 4
        r["intervals_%s_bytes" % name] = nbytes
        r["intervals_%s_GBps" % name] = nbytes / ms / 1e6
        r["intervals_%s_fraction_of_hbm" % name] = r["intervals_%s_GBps" % name] / (HBM_TBS * 1e3)
        r["intervals_%s_over_classes_1" % name] = ms / t["classes_1"]
        r["torch_over_intervals_%s" % name] = t["torch_" + name] / ms
        # a check of what was timed: the kernel against the torch formulation on a slice
        lo, hi, out = sets[name]
        r["intervals_%s_check_equal" % name] = bool(torch.equal(out[:64], marginals_torch(hm[:64], lo[:64], hi[:64])))
    r["classes_1_GBps"] = (map_bytes + B * nz * 20) / t["classes_1"] / 1e6
    r["classes_1_fraction_of_hbm"] = r["classes_1_GBps"] / (HBM_TBS * 1e3)

    # the 64-bit statistics kernels on the marginals (through the Python entries: they are small)
    q, _, _ = line_products.quantiles()
    for name in sets:
        marg = sets[name][2]
        t64 = alternating({"products": lambda: hitmap.moments(marg, lmp, hw, q),
                           "classes_4": lambda: hitmap.class_probability(marg, lmp, hw, [-3.0, -2.5, -2.0, -1.0], [0.3, 0.3, 0.4, 0.5])}, a.reps)
        r["products_i64_%s_ms" % name] = t64["products"]
        r["classes_4_i64_%s_ms" % name] = t64["classes_4"]
    r["device"] = torch.cuda.get_device_name(0)
    for k, v in r.items():
        print("%s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
