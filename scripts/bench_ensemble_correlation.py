"""Correlation between depth cells of an ensemble (gbp_ensemble_correlation) against the formulation a user would
otherwise write in torch: ensembles.realisations -> log10 -> centre -> torch.bmm(d^T, d) -> normalise -> gather the band; or, instead of
the Gram matrix, W + 1 shifted elementwise product sums over the series.  Both are timed and the faster one is the yardstick.

The synthetic ensembles of bench_ensemble_diagnostics.py: B soundings, K = 30, n_keep = 256 and 4 096, 440 depth cells, one chain (both
halves: n = n_keep used rows).  The C entry is timed on preallocated buffers with device events, medians after warm-up rounds; the
yardsticks run in the same process, alternating with it, on as many soundings as fit the device, and are compared per sounding.  At
band 64 the outputs must agree within the bound of tests/test_ensemble_correlation_gpu.py and the kernel must be the faster one: the
script says so in its JSON (``condition_met``) and exits non-zero otherwise.  The full band (W = 439) and k_band_runs are timed too,
with no bar.  Writes one JSON file.

    python scripts/bench_ensemble_correlation.py [--soundings 1024] [--rounds 5] [--out profiles/ensemble_correlation/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_ensemble_diagnostics import K, N_DEPTH, events_ms, synthetic      # noqa: E402
from geobipy_amd import _lib, ensembles      # noqa: E402

BAND, U = 64, 2.0 ** -52


def centred(ens, depth_edges):
    x = ensembles.realisations(ens, depth_edges)                         # [B, n, V], log10: the series written out
    return x, x - x.mean(dim=1, keepdim=True)


def yardstick_bmm(ens, depth_edges, W):
    """band [B, V, W + 1], sd [B, V] from the full Gram matrix (rocBLAS batched DGEMM)."""
    x, d = centred(ens, depth_edges)
    B, n, V = x.shape
    C = torch.bmm(d.transpose(1, 2), d) / (n - 1.0)
    sd = torch.sqrt(torch.diagonal(C, dim1=1, dim2=2))
    R = C / (sd[:, :, None] * sd[:, None, :])
    col = torch.arange(V, device=x.device)[:, None] + torch.arange(W + 1, device=x.device)[None, :]
    band = torch.gather(R, 2, col.clamp(max=V - 1)[None].expand(B, V, W + 1))
    return torch.where(col[None] < V, band, torch.full((), float("nan"), dtype=band.dtype, device=band.device)), sd, x


def yardstick_shifts(ens, depth_edges, W):
    """The same from W + 1 shifted elementwise product sums: no Gram matrix, W + 1 passes over the series."""
    x, d = centred(ens, depth_edges)
    B, n, V = x.shape
    sd = torch.sqrt((d * d).sum(dim=1) / (n - 1.0))
    band = torch.full((B, V, W + 1), float("nan"), dtype=x.dtype, device=x.device)
    for j in range(W + 1):
        band[:, :V - j, j] = (d[:, :, :V - j] * d[:, :, j:]).sum(dim=1) / (n - 1.0) / (sd[:, :V - j] * sd[:, j:])
    return band, sd, x


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--soundings", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 4096])
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ensemble_correlation", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ensemble_correlation needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    B = a.soundings
    depth_edges = np.arange(N_DEPTH + 1) * (165.0 / N_DEPTH)
    z = torch.as_tensor(ensembles.centres(depth_edges)).to(dev)
    result = dict(device=torch.cuda.get_device_name(dev), soundings=B, K=K, n_depth=N_DEPTH, band=BAND, rounds=a.rounds, warmup=a.warmup, sizes={})
    stream = torch.cuda.current_stream(dev).cuda_stream
    for n_keep in a.sizes:
        ens = synthetic(B, n_keep, dev, seed=n_keep)
        start_np, m_np, n_np, _ = ensembles.segments(ens.count.cpu().numpy()[:, None], n_keep)
        start, seg_m, seg_n = (torch.as_tensor(v).to(dev) for v in (start_np, m_np, n_np))
        stats = torch.empty((B, 2, N_DEPTH), dtype=torch.float64, device=dev)
        band = torch.empty((B, N_DEPTH, BAND + 1), dtype=torch.float64, device=dev)
        full = torch.empty((B, N_DEPTH, N_DEPTH), dtype=torch.float64, device=dev)
        up, down = (torch.empty((B, N_DEPTH), dtype=torch.int32, device=dev) for _ in range(2))
        closed = torch.empty((B, 2, N_DEPTH), dtype=torch.uint8, device=dev)

        def kernel(W=BAND, out=band):
            _lib.check(lib.gbp_ensemble_correlation(B, n_keep, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), N_DEPTH, z.data_ptr(),
                                                    2, start.data_ptr(), seg_m.data_ptr(), seg_n.data_ptr(), W, 1, stats.data_ptr(), out.data_ptr(), stream))

        def runs():
            _lib.check(lib.gbp_band_runs(B, N_DEPTH, BAND, band.data_ptr(), 0.5, up.data_ptr(), down.data_ptr(), closed.data_ptr(), stream))
        # the yardsticks' block: the series, its log10, its centred copy and a product, twice (the last answer is kept for the comparison),
        # and the Gram matrix with its normalised copy
        per = 8.0 * (6.0 * n_keep * N_DEPTH + 4 * N_DEPTH * N_DEPTH)
        Bt = int(max(1, min(B, 0.5 * torch.cuda.mem_get_info(dev)[0] // per)))
        while True:
            part = ensembles.Ensemble(ens.k[:Bt], ens.edges[:Bt], ens.sigma[:Bt], ens.misfit[:Bt], ens.count[:Bt], 1, ens.log_mean_prior[:Bt])
            try:
                for _ in range(a.warmup):
                    kernel()
                    kernel(N_DEPTH - 1, full)
                    runs()
                    yardstick_bmm(part, depth_edges, BAND)
                    yardstick_shifts(part, depth_edges, BAND)
                torch.cuda.synchronize(dev)
                break
            except torch.cuda.OutOfMemoryError:
                if Bt == 1:
                    raise
                torch.cuda.empty_cache()
                Bt = max(1, Bt // 2)
        t = dict(kernel=[], full=[], runs=[], bmm=[], shifts=[])
        for _ in range(a.rounds):                                        # alternating, in one process
            t["kernel"].append(events_ms(kernel, dev)[0])
            ms, want = events_ms(lambda: yardstick_bmm(part, depth_edges, BAND), dev)
            t["bmm"].append(ms)
            t["shifts"].append(events_ms(lambda: yardstick_shifts(part, depth_edges, BAND)[0].shape, dev)[0])
            t["runs"].append(events_ms(runs, dev)[0])
            t["full"].append(events_ms(lambda: kernel(N_DEPTH - 1, full), dev)[0])
        med = {n: float(np.median(v)) for n, v in t.items()}
        # agreement at band 64 within the test's bound: eps = 8 (n + 8) U (1 + max |x| / min sd), per sounding
        y_band, y_sd, x = want
        live = y_sd > 0
        r = x.abs().amax(dim=(1, 2)) / torch.where(live, y_sd, torch.full_like(y_sd, float("inf"))).amin(dim=1)
        eps = 8.0 * (n_keep + 8) * U * (1.0 + r)
        got = band[:Bt]
        same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(y_band)))
        diff = torch.nan_to_num((got - y_band).abs(), nan=0.0).amax(dim=(1, 2)) / eps
        diff_full = torch.nan_to_num((full[:Bt, :, :BAND + 1] - got).abs(), nan=0.0).max()
        worst = float(diff.max())
        per_k, per_y = med["kernel"] / B, min(med["bmm"], med["shifts"]) / Bt
        live_strips = int((stats[:, 1].reshape(B, -1)[:, :(N_DEPTH // 64) * 64].reshape(B, -1, 64) > 0).any(dim=2).sum()) + \
            int((stats[:, 1, (N_DEPTH // 64) * 64:] > 0).any(dim=1).sum())
        mfma_fma = live_strips * 4.0 * 5 * 256 * n_keep                  # issued at band 64: 4 tile rows x 5 tiles x 16 x 16 cells x n rows
        entry = dict(kernel_ms=t["kernel"], kernel_full_band_ms=t["full"], band_runs_ms=t["runs"], torch_bmm_ms=t["bmm"], torch_shifts_ms=t["shifts"],
                     torch_soundings=Bt, kernel_ms_per_sounding=per_k, torch_bmm_ms_per_sounding=med["bmm"] / Bt,
                     torch_shifts_ms_per_sounding=med["shifts"] / Bt, yardstick="bmm" if med["bmm"] <= med["shifts"] else "shifts",
                     ratio_yardstick_over_kernel=per_y / per_k, kernel_full_band_ms_per_sounding=med["full"] / B,
                     ratio_bmm_over_kernel_full_band=(med["bmm"] / Bt) / (med["full"] / B), band_runs_ms_median=med["runs"],
                     live_strips=live_strips, kernel_mfma_fma_per_s=mfma_fma / (med["kernel"] * 1e-3),
                     worst_difference_over_bound=worst, nan_patterns_equal=same_nan, full_band_first_columns_max_difference=float(diff_full),
                     condition_met=bool(per_k < per_y and worst <= 1.0 and same_nan), series_bytes_avoided=float(B) * n_keep * N_DEPTH * 8)
        result["sizes"][str(n_keep)] = entry
        print("n_keep %5d: kernel %.3f ms / %d soundings (full band %.3f ms, runs %.3f ms); torch bmm %.3f ms, shifts %.3f ms / %d soundings; per sounding x%.2f; "
              "worst difference %.3g of the bound; %.3g MFMA FMA/s" % (n_keep, med["kernel"], B, med["full"], med["runs"], med["bmm"], med["shifts"], Bt,
                                                                   entry["ratio_yardstick_over_kernel"], worst, entry["kernel_mfma_fma_per_s"]))
        del ens, part, want, got, full, band, y_band, y_sd, x
        torch.cuda.empty_cache()
    result["condition_met"] = all(v["condition_met"] for v in result["sizes"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({n: {"ratio": v["ratio_yardstick_over_kernel"], "condition_met": v["condition_met"]} for n, v in result["sizes"].items()}))
    return 0 if result["condition_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
