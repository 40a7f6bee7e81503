"""Time of the replicate-pooling kernel (csrc/gbp_hitmap.h k_hitmap_pool) on synthetic layered hit maps -- 8 192 maps of 250 x 440 as
2 048 soundings x 4 chains -- against k_hitmap_classes at K = 1 on the same maps (the project's fastest single read of them) and the
torch formulation (``view(S, C, nv, nz).sum(1)`` plus the moment and entropy sums):

    python scripts/bench_replicates.py [--S 2048] [--C 4] [--reps 20] [--out profiles/replicates/bench.json]

Every kernel is launched through its C entry on preallocated buffers and timed with device events, one launch per event pair, the
candidates alternating inside each repetition of one process; the figures are medians after a warm-up.  The bar (the interval kernel's
precedent): pool_ms <= 1.5 x classes_1_ms x (C + 1) / C -- the pooled map's write on top of the read -- and faster than torch.  Prints
one line per measurement and writes them as JSON to --out."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_intervals import alternating  # noqa: E402
from bench_line_products import HBM_TBS, layered_maps  # noqa: E402
from geobipy_amd import _lib, line_products, replicates  # noqa: E402


def pool_torch(hm, C, hw):
    """The torch formulation of what the kernel accumulates: the pooled map, and per chain the column totals, the two moments and the
    entropy sum (the per-cell diagnostics that follow are elementwise on [S, C, nz] and small)."""
    R, nv, nz = hm.shape
    S = R // C
    pooled = hm.view(S, C, nv, nz).sum(dim=1, dtype=torch.int32)
    x = (((torch.arange(nv, dtype=torch.float64, device=hm.device) + 0.5) / nv) * (2.0 * hw) - hw)[None, :, None]
    hf = hm.to(torch.float64)
    n = hm.sum(dim=1, dtype=torch.int64)
    hx = hf * x
    a = hx.sum(dim=1)
    q = (hx * x).sum(dim=1)
    e = torch.xlogy(hf, hf).sum(dim=1)
    pf = pooled.to(torch.float64)
    ep = torch.xlogy(pf, pf).sum(dim=1)
    return pooled, n, a, q, e, ep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, C, nv, nz, hw = a.S, a.C, 250, 440, 2.3
    R = S * C
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    hm = layered_maps(R, nv, nz, dev)
    lmp = torch.full((R,), -2.0 * line_products.LN10, dtype=torch.float64, device=dev)
    use = torch.ones((S, C), dtype=torch.int32, device=dev)
    map_bytes = R * nv * nz * 4
    r = dict(S=S, C=C, maps=R, n_value=nv, n_depth=nz, map_bytes=map_bytes, reps=a.reps)

    pooled = torch.empty((S, nv, nz), dtype=torch.int32, device=dev)
    n_used = torch.empty((S, nz), dtype=torch.int32, device=dev)
    chain_mean = torch.empty((S, C, nz), dtype=torch.float64, device=dev)
    rhat = torch.empty((S, nz), dtype=torch.float64, device=dev)
    jsd = torch.empty((S, nz), dtype=torch.float64, device=dev)

    def pool():
        _lib.check(lib.gbp_hitmap_pool(S, C, nv, nz, hm.data_ptr(), use.data_ptr(), hw, pooled.data_ptr(), n_used.data_ptr(), chain_mean.data_ptr(),
                                       rhat.data_ptr(), jsd.data_ptr(), stream))

    mu, sd = (ctypes.c_double * 1)(-2.0), (ctypes.c_double * 1)(0.4)
    prob = torch.empty((R, 1, nz), dtype=torch.float64, device=dev)
    best = torch.empty((R, nz), dtype=torch.int32, device=dev)
    best_p = torch.empty((R, nz), dtype=torch.float64, device=dev)

    def classes_1():
        _lib.check(lib.gbp_hitmap_classes(R, nv, nz, hm.data_ptr(), lmp.data_ptr(), hw, 1, mu, sd, prob.data_ptr(), best.data_ptr(), best_p.data_ptr(),
                                          stream))

    t = alternating({"pool": pool, "classes_1": classes_1}, a.reps)
    t.update(alternating({"torch": lambda: pool_torch(hm, C, hw)}, max(3, a.reps // 4), warmup=1))
    for k, ms in t.items():
        r[k + "_ms"] = ms
    nbytes = map_bytes + S * nv * nz * 4 + S * nz * (4 + 8 + 8 + 8 * C) + S * C * 4
    r["pool_bytes"] = nbytes
    r["pool_GBps"] = nbytes / t["pool"] / 1e6
    r["pool_fraction_of_hbm"] = r["pool_GBps"] / (HBM_TBS * 1e3)
    r["classes_1_GBps"] = (map_bytes + R * nz * 20) / t["classes_1"] / 1e6
    r["classes_1_fraction_of_hbm"] = r["classes_1_GBps"] / (HBM_TBS * 1e3)
    r["pool_over_classes_1"] = t["pool"] / t["classes_1"]
    r["bar_ms"] = 1.5 * t["classes_1"] * (C + 1) / C
    r["pool_meets_the_bar"] = bool(t["pool"] <= r["bar_ms"] and t["pool"] < t["torch"])
    r["torch_over_pool"] = t["torch"] / t["pool"]
    # a check of what was timed: the kernel against the host rule on a slice, and the pooled map against torch's sum
    k = 8 * C
    ref = replicates.pool_reference(hm[:k].cpu().numpy(), C, None, hw)
    r["pool_check_pooled_equal"] = bool(torch.equal(pooled, hm.view(S, C, nv, nz).sum(dim=1, dtype=torch.int32)))
    fin = torch.as_tensor(ref["rhat"]).isfinite()
    r["pool_check_rhat_max_rel"] = float(((rhat[:8].cpu() - torch.as_tensor(ref["rhat"])).abs() / torch.as_tensor(ref["rhat"]).abs())[fin].max()) if fin.any() else 0.0
    fin = torch.as_tensor(ref["jsd"]).isfinite()
    r["pool_check_jsd_max_abs"] = float((jsd[:8].cpu() - torch.as_tensor(ref["jsd"])).abs()[fin].max()) if fin.any() else 0.0
    r["device"] = torch.cuda.get_device_name(0)
    for k_, v in r.items():
        print("%s: %s" % (k_, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
