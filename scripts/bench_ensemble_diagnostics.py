"""Chain diagnostics of an ensemble (gbp_ensemble_diagnostics) against the formulation a user would otherwise write in
torch: ensembles.realisations -> log10 -> centred torch.fft.rfft autocovariance -> the same pair walk with cummin / cumsum.

Synthetic ensembles: B soundings, K = 30, an AR(1) walk in the layers' log10 conductivities over the slots with births and deaths,
n_keep = 256 and 4 096, 440 depth cells, one chain (M = 2 split halves), max_lag 255.  The C entry is timed on preallocated buffers with
device events after warm-up; the yardstick runs in the same process, alternating with it, on as many soundings as fit the device
(its [B, n, n_depth] series and the FFT workspace: all of them where they fit, half as many after an out-of-memory error), and
the two are compared per sounding.  Writes one JSON file.

    python scripts/bench_ensemble_diagnostics.py [--soundings 1024] [--rounds 5] [--out profiles/ensemble_diagnostics/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from geobipy_amd import _lib, ensembles      # noqa: E402

K, N_DEPTH, MAX_LAG = 30, 440, 255


def synthetic(B, n_keep, dev, seed):
    """An Ensemble of B full chains: interfaces drawn from a pool of K - 1 depths per sounding (the k - 1 a model uses are a fixed
    random subset, so births and deaths add and remove interfaces all over the section), log10 conductivities AR(1) with phi = 0.9."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float64)      # noqa: E731
    pool = torch.rand((B, K - 1), generator=g, device=dev, dtype=torch.float64) * 150.0 + 1.0
    rank = torch.argsort(torch.rand((B, K - 1), generator=g, device=dev), dim=1)
    steps = torch.randint(-1, 2, (B, n_keep), generator=g, device=dev)
    k = torch.clamp(8 + torch.cumsum(steps, dim=1), 1, K).to(torch.int32)
    edges = torch.where(rank[:, None, :] < (k[:, :, None] - 1), pool[:, None, :], torch.full((), float("inf"), dtype=torch.float64, device=dev))
    edges = torch.cat([torch.sort(edges, dim=2).values, torch.full((B, n_keep, 1), float("inf"), dtype=torch.float64, device=dev)], dim=2)
    ls = torch.empty((B, n_keep, K), dtype=torch.float64, device=dev)
    cur = rnd(B, K)
    for s in range(n_keep):
        cur = 0.9 * cur + (1.0 - 0.81) ** 0.5 * rnd(B, K)
        ls[:, s] = cur
    sigma = torch.where(torch.arange(K, device=dev)[None, None, :] < k[:, :, None], 10.0 ** (0.6 * ls - 1.5),
                        torch.full((), float("nan"), dtype=torch.float64, device=dev))
    misfit = torch.rand((B, n_keep), generator=g, device=dev, dtype=torch.float64) * 20.0 + 1.0
    return ensembles.Ensemble(k, edges.contiguous(), sigma.contiguous(), misfit, (k > 0).sum(dim=1), 1, torch.zeros(B, dtype=torch.float64, device=dev))


def torch_yardstick(ens, depth_edges, max_lag):
    """tau, ess, rhat, mcse [B, n_depth] of one chain split in two halves, in torch: the series is written out and its autocovariance
    comes from a zero-padded FFT."""
    x = ensembles.realisations(ens, depth_edges)                         # [B, n, V], log10
    B, n, V = x.shape
    N = n // 2
    L = int(ensembles.lag_count(N, max_lag))
    seg = x[:, :2 * N].reshape(B, 2, N, V)
    mean = seg.mean(dim=2)
    d = seg - mean[:, :, None, :]
    n_fft = 1 << int(np.ceil(np.log2(2 * N)))
    F = torch.fft.rfft(d, n=n_fft, dim=2)
    acov = torch.fft.irfft(F * F.conj(), n=n_fft, dim=2)[:, :, :L + 1] / N
    A = acov.mean(dim=1) * (N / (N - 1.0))                               # [B, L + 1, V]
    W = A[:, 0]
    Bn = mean.var(dim=1, unbiased=True)
    vp = W * ((N - 1.0) / N) + Bn
    rho = 1.0 - (W[:, None] - A) / vp[:, None]
    rho[:, 0] = 1.0
    P = rho[:, 0::2] + rho[:, 1::2]                                      # [B, pairs, V]
    positive = P > 0
    positive[:, 0] = True
    open_ = torch.cumprod(positive.to(torch.int8), dim=1).bool()
    S = torch.where(open_, torch.cummin(P, dim=1).values, torch.zeros((), dtype=P.dtype, device=P.device)).sum(dim=1)
    total = 2.0 * N
    tau = torch.clamp(2.0 * S - 1.0, min=1.0 / np.log10(total))
    ess = total / tau
    return dict(tau=tau, ess=ess, rhat=torch.sqrt(vp / W), mcse=torch.sqrt(vp / ess), sd=torch.sqrt(vp), mean=mean.mean(dim=1))


def events_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--soundings", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 4096])
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ensemble_diagnostics", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ensemble_diagnostics needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    B = a.soundings
    depth_edges = np.arange(N_DEPTH + 1) * (165.0 / N_DEPTH)
    z = torch.as_tensor(ensembles.centres(depth_edges)).to(dev)
    result = dict(device=torch.cuda.get_device_name(dev), soundings=B, K=K, n_depth=N_DEPTH, max_lag=MAX_LAG, rounds=a.rounds, sizes={})
    for n_keep in a.sizes:
        ens = synthetic(B, n_keep, dev, seed=n_keep)
        start_np, m_np, n_np, _ = ensembles.segments(ens.count.cpu().numpy()[:, None], n_keep)
        start, seg_m, seg_n = (torch.as_tensor(v).to(dev) for v in (start_np, m_np, n_np))
        stats = torch.empty((B, 6, N_DEPTH), dtype=torch.float64, device=dev)
        pairs = torch.empty((B, N_DEPTH), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def kernel():
            _lib.check(lib.gbp_ensemble_diagnostics(B, n_keep, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), N_DEPTH, z.data_ptr(),
                                                    2, start.data_ptr(), seg_m.data_ptr(), seg_n.data_ptr(), MAX_LAG, stats.data_ptr(), pairs.data_ptr(),
                                                    None, stream))
        # the yardstick's block: the series, its centred copy, the spectrum, the power spectrum and the padded autocovariance
        n_fft = 1 << int(np.ceil(np.log2(n_keep)))
        per = N_DEPTH * 8 * (3 * n_keep + 2 * 2 * (n_fft + 2) + 2 * n_fft) * 1.5
        free = torch.cuda.mem_get_info(dev)[0]
        Bt = int(max(1, min(B, 0.5 * free // per)))                      # as many soundings as fit (the estimate is generous) ...
        while True:
            part = ensembles.Ensemble(ens.k[:Bt], ens.edges[:Bt], ens.sigma[:Bt], ens.misfit[:Bt], ens.count[:Bt], 1, ens.log_mean_prior[:Bt])
            try:
                for _ in range(2):                                       # warm-up of both: code objects, FFT plans
                    kernel()
                    want = torch_yardstick(part, depth_edges, MAX_LAG)
                torch.cuda.synchronize(dev)
                break
            except torch.cuda.OutOfMemoryError:                          # ... and half as many where it was not generous enough
                if Bt == 1:
                    raise
                want = None
                torch.cuda.empty_cache()
                Bt = max(1, Bt // 2)
        t_kernel, t_torch = [], []
        for _ in range(a.rounds):                                        # alternating, in one process
            t_kernel.append(events_ms(kernel, dev)[0])
            ms, want = events_ms(lambda: torch_yardstick(part, depth_edges, MAX_LAG), dev)
            t_torch.append(ms)
        got = dict(zip(ensembles.STAT_NAMES, stats[:Bt].unbind(dim=1)))
        live = torch.isfinite(got["tau"])
        same_pairs = float(((got["tau"] - want["tau"]).abs() <= 1e-9 * want["tau"])[live].double().mean())
        worst = {n: float(((got[n] - want[n]).abs() / want[n].abs())[live].max()) for n in ("sd", "rhat")}
        N = n_keep // 2
        L = int(ensembles.lag_count(N, MAX_LAG))
        tiles_live = int((torch.isfinite(stats[:, 3]).reshape(B, -1)[:, : (N_DEPTH // 64) * 64].reshape(B, -1, 64).any(dim=2)).sum()) + \
            int(torch.isfinite(stats[:, 3, (N_DEPTH // 64) * 64:]).any(dim=1).sum())
        fma = tiles_live * 2.0 * N * (16 * ((L + 16) // 16)) * 64       # what the kernel issues: padded lags, 64 lanes per tile
        k_ms, y_ms = float(np.median(t_kernel)), float(np.median(t_torch))
        entry = dict(kernel_ms=t_kernel, torch_ms=t_torch, torch_soundings=Bt, kernel_ms_per_sounding=k_ms / B, torch_ms_per_sounding=y_ms / Bt,
                     ratio_torch_over_kernel=(y_ms / Bt) / (k_ms / B), kernel_fma_per_s=fma / (k_ms * 1e-3), live_tiles=tiles_live,
                     share_of_cells_with_tau_within_1e9=same_pairs, worst_relative_difference=worst,
                     series_bytes_avoided=float(B) * n_keep * N_DEPTH * 8)
        result["sizes"][str(n_keep)] = entry
        print("n_keep %5d: kernel %.3f ms / %d soundings, torch %.3f ms / %d soundings, per sounding x%.2f; %.3g FMA/s; tau equal in %.4f of the cells"
              % (n_keep, k_ms, B, y_ms, Bt, entry["ratio_torch_over_kernel"], entry["kernel_fma_per_s"], same_pairs))
        del ens, part, want, got
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({n: {"ratio": v["ratio_torch_over_kernel"]} for n, v in result["sizes"].items()}))
    return result


if __name__ == "__main__":
    main()
