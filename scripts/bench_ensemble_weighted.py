"""Weighted products within the columns of an ensemble (gbp_ensemble_weighted) against the formulation a user would
otherwise write in torch: ensembles.realisations -> log10 -> torch.sort along the model axis -> a gather of the weights -> cumsum ->
searchsorted for the quantiles and the thresholds, plus the two weighted moment sums.

The synthetic ensembles of scripts/bench_ensemble_diagnostics.py: B soundings, K = 30, 440 depth cells, n = 256 and 1 024 models (every
slot listed once, in order), random weights with a tenth of them 0 (``ensembles.quantise_weights``), three probabilities and two
thresholds.  The C entry is timed on preallocated buffers with device events after 2 warm-up rounds; the yardstick runs in the same
process, taking turns with it, on as many soundings as fit the device, and the two are compared per sounding; the quantiles must be
torch.equal.  The condition: the kernel is no slower than the yardstick at both sizes.  Writes one JSON file; exits 1 when the
condition is not met.

    python scripts/bench_ensemble_weighted.py [--soundings 1024] [--rounds 5] [--out profiles/ensemble_weighted/bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ensemble_diagnostics import K, N_DEPTH, events_ms, synthetic      # noqa: E402
from geobipy_amd import _lib, ensembles      # noqa: E402

PROBABILITIES = (0.05, 0.5, 0.95)
THRESHOLDS = (-0.5, 0.5)
WARMUP = 2


def torch_yardstick(ens, depth_edges, q, p, thr):
    """quantile f64 [B, n_p, V], above int64 [B, n_t, V], mean, sd f64 [B, V] of every slot under the multiplicities q [B, n], in torch."""
    x = ensembles.realisations(ens, depth_edges).transpose(1, 2).contiguous()      # [B, V, n], log10
    B, V, n = x.shape
    s, idx = torch.sort(x, dim=2)
    C = torch.cumsum(torch.gather(q[:, None, :].expand(B, V, n), 2, idx), dim=2)
    W = C[:, :, -1:]
    Wf = W.to(torch.float64)
    target = torch.clamp(p[None, None, :] * Wf, min=1.0)
    quantile = torch.gather(s, 2, torch.searchsorted(C.to(torch.float64), target).clamp(max=n - 1))
    lo = torch.searchsorted(s, thr[None, None, :].expand(B, V, -1).contiguous())
    below = torch.where(lo > 0, torch.gather(C, 2, (lo - 1).clamp(min=0)), torch.zeros((), dtype=torch.int64, device=x.device))
    qf = q.to(torch.float64)[:, None, :]
    mean = (qf * x).sum(dim=2, keepdim=True) / Wf
    d = x - mean
    sd = torch.sqrt((qf * d * d).sum(dim=2, keepdim=True) / Wf)
    return quantile.transpose(1, 2), (W - below).transpose(1, 2), mean[:, :, 0], sd[:, :, 0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--soundings", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ensemble_weighted", "bench.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ensemble_weighted needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    B = a.soundings
    depth_edges = np.arange(N_DEPTH + 1) * (165.0 / N_DEPTH)
    z = torch.as_tensor(ensembles.centres(depth_edges)).to(dev)
    probs, thrs = (ctypes.c_double * len(PROBABILITIES))(*PROBABILITIES), (ctypes.c_double * len(THRESHOLDS))(*THRESHOLDS)
    p_t, thr_t = torch.tensor(PROBABILITIES, dtype=torch.float64, device=dev), torch.tensor(THRESHOLDS, dtype=torch.float64, device=dev)
    result = dict(device=torch.cuda.get_device_name(dev), soundings=B, K=K, n_depth=N_DEPTH, probabilities=PROBABILITIES, thresholds=THRESHOLDS,
                  rounds=a.rounds, warmup=WARMUP, sizes={})
    met = True
    for n in a.sizes:
        ens = synthetic(B, n, dev, seed=n)
        g = torch.Generator(device=dev).manual_seed(n + 1)
        w = torch.rand((B, n), generator=g, device=dev, dtype=torch.float64)
        w = torch.where(torch.rand((B, n), generator=g, device=dev) < 0.1, torch.zeros_like(w), w)
        n_used = torch.full((B,), n, dtype=torch.int32, device=dev)
        q = ensembles.quantise_weights(w, n_used)
        rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(B, n).contiguous()
        total = torch.empty(B, dtype=torch.int64, device=dev)
        quantile = torch.empty((B, len(PROBABILITIES), N_DEPTH), dtype=torch.float64, device=dev)
        above = torch.empty((B, len(THRESHOLDS), N_DEPTH), dtype=torch.int64, device=dev)
        stats = torch.empty((B, 2, N_DEPTH), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def kernel():
            _lib.check(lib.gbp_ensemble_weighted(B, n, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), N_DEPTH, z.data_ptr(), n,
                                                 rows.data_ptr(), n_used.data_ptr(), q.data_ptr(), len(PROBABILITIES), probs, len(THRESHOLDS), thrs,
                                                 total.data_ptr(), quantile.data_ptr(), above.data_ptr(), stats.data_ptr(), stream))
        # the yardstick's block: the series, its transpose, the sorted copy and its index array, the gathered weights, two cumulated copies
        per = N_DEPTH * n * 8 * 10 * 1.5
        Bt = int(max(1, min(B, 0.5 * torch.cuda.mem_get_info(dev)[0] // per)))
        while True:
            part = ensembles.Ensemble(ens.k[:Bt], ens.edges[:Bt], ens.sigma[:Bt], ens.misfit[:Bt], ens.count[:Bt], 1, ens.log_mean_prior[:Bt])
            try:
                for _ in range(WARMUP):
                    kernel()
                    want = torch_yardstick(part, depth_edges, q[:Bt], p_t, thr_t)
                torch.cuda.synchronize(dev)
                break
            except torch.cuda.OutOfMemoryError:
                if Bt == 1:
                    raise
                want = None
                torch.cuda.empty_cache()
                Bt = max(1, Bt // 2)
        t_kernel, t_torch = [], []
        for _ in range(a.rounds):                                        # taking turns, in one process
            t_kernel.append(events_ms(kernel, dev)[0])
            ms, want = events_ms(lambda: torch_yardstick(part, depth_edges, q[:Bt], p_t, thr_t), dev)
            t_torch.append(ms)
        equal = bool(torch.equal(quantile[:Bt], want[0]))
        above_equal = bool(torch.equal(above[:Bt], want[1]))
        moments = float(max((stats[:Bt, 0] - want[2]).abs().max(), (stats[:Bt, 1] - want[3]).abs().max()))
        k_ms, y_ms = float(np.median(t_kernel)), float(np.median(t_torch))
        ratio = (y_ms / Bt) / (k_ms / B)
        result["sizes"][str(n)] = dict(torch_soundings=Bt, kernel_ms=t_kernel, torch_ms=t_torch, kernel_ms_per_sounding=k_ms / B,
                                       torch_ms_per_sounding=y_ms / Bt, ratio_torch_over_kernel=ratio, quantiles_equal=equal, above_equal=above_equal,
                                       moments_max_abs_difference=moments)
        met = met and equal and ratio >= 1.0
        print("n %5d: kernel %.3f ms / %d soundings, torch %.3f ms / %d soundings, per sounding x%.2f; quantiles equal: %s, above equal: %s, moments within %.2e"
              % (n, k_ms, B, y_ms, Bt, ratio, equal, above_equal, moments))
        del want, part, ens, quantile, above, stats
        torch.cuda.empty_cache()
    result["condition_met"] = bool(met)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({n: v["ratio_torch_over_kernel"] for n, v in result["sizes"].items()}))
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
