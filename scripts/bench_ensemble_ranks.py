"""Ranks within the columns of an ensemble (gbp_ensemble_ranks) against the formulation a user would otherwise write in
torch: ensembles.realisations -> torch.sort along the slot axis -> two torch.searchsorted (folded: the median from the sorted
series, |x - med|, a second sort); and the whole pipeline ensembles.rank_diagnostics beside ensembles.diagnostics.

The synthetic ensembles of scripts/bench_ensemble_diagnostics.py: B soundings, K = 30, n_keep = 256 and 4 096, 440 depth cells, one
chain (M = 2 split halves: every slot is a used row).  The C entry (counts and three probabilities, unfolded and folded) is timed on
preallocated buffers with device events after warm-up; the yardstick runs in the same process, taking turns with it, on as many
soundings as fit the device (its series, the sorted copy and two count arrays), and the two are compared per sounding; the counts
must be torch.equal.  Writes one JSON file.

    python scripts/bench_ensemble_ranks.py [--soundings 1024] [--rounds 5] [--out profiles/ensemble_ranks/bench.json]
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
from bench_ensemble_diagnostics import K, MAX_LAG, N_DEPTH, events_ms, synthetic      # noqa: E402
from geobipy_amd import _lib, ensembles      # noqa: E402

PROBABILITIES = (0.05, 0.5, 0.95)


def torch_yardstick(ens, depth_edges, fold):
    """less, leq int32 [B, n_depth, n] (the slot axis last, as torch.searchsorted wants it) of every slot of full chains, in torch."""
    x = ensembles.realisations(ens, depth_edges).transpose(1, 2).contiguous()      # [B, V, n], log10
    s = torch.sort(x, dim=2).values
    if fold:
        n = x.shape[2]
        med = 0.5 * (s[:, :, (n - 1) // 2] + s[:, :, n // 2])
        x = (x - med[:, :, None]).abs()
        s = torch.sort(x, dim=2).values
    return torch.searchsorted(s, x, right=False, out_int32=True), torch.searchsorted(s, x, right=True, out_int32=True)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--soundings", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 4096])
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ensemble_ranks", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ensemble_ranks needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    B = a.soundings
    depth_edges = np.arange(N_DEPTH + 1) * (165.0 / N_DEPTH)
    z = torch.as_tensor(ensembles.centres(depth_edges)).to(dev)
    probs = (ctypes.c_double * len(PROBABILITIES))(*PROBABILITIES)
    result = dict(device=torch.cuda.get_device_name(dev), soundings=B, K=K, n_depth=N_DEPTH, probabilities=PROBABILITIES, rounds=a.rounds, sizes={})
    for n_keep in a.sizes:
        ens = synthetic(B, n_keep, dev, seed=n_keep)
        start_np, m_np, n_np, _ = ensembles.segments(ens.count.cpu().numpy()[:, None], n_keep)
        assert np.all(m_np * n_np == n_keep)                             # every slot is a used row: the yardstick ranks them all
        start, seg_m, seg_n = (torch.as_tensor(v).to(dev) for v in (start_np, m_np, n_np))
        less, leq = (torch.empty((B, n_keep, N_DEPTH), dtype=torch.int32, device=dev) for _ in range(2))
        order = torch.empty((B, len(PROBABILITIES), 2, N_DEPTH), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def kernel(fold):
            _lib.check(lib.gbp_ensemble_ranks(B, n_keep, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), N_DEPTH, z.data_ptr(), 2,
                                              start.data_ptr(), seg_m.data_ptr(), seg_n.data_ptr(), int(fold), len(PROBABILITIES), probs,
                                              less.data_ptr(), leq.data_ptr(), order.data_ptr(), None, stream))
        # the yardstick's block: the series, its transpose, the sorted copy (and torch.sort's index array), two count arrays
        per = N_DEPTH * n_keep * (8 * 4 + 8 + 4 * 2) * 1.5
        Bt = int(max(1, min(B, 0.5 * torch.cuda.mem_get_info(dev)[0] // per)))
        while True:
            part = ensembles.Ensemble(ens.k[:Bt], ens.edges[:Bt], ens.sigma[:Bt], ens.misfit[:Bt], ens.count[:Bt], 1, ens.log_mean_prior[:Bt])
            try:
                for fold in (False, True):                               # warm-up of both
                    kernel(fold)
                    want = torch_yardstick(part, depth_edges, fold)
                torch.cuda.synchronize(dev)
                break
            except torch.cuda.OutOfMemoryError:
                if Bt == 1:
                    raise
                want = None
                torch.cuda.empty_cache()
                Bt = max(1, Bt // 2)
        entry = dict(torch_soundings=Bt)
        for fold in (False, True):
            t_kernel, t_torch = [], []
            for _ in range(a.rounds):                                    # taking turns, in one process
                t_kernel.append(events_ms(lambda: kernel(fold), dev)[0])
                ms, want = events_ms(lambda: torch_yardstick(part, depth_edges, fold), dev)
                t_torch.append(ms)
            equal = bool(torch.equal(less[:Bt].transpose(1, 2), want[0]) and torch.equal(leq[:Bt].transpose(1, 2), want[1]))
            k_ms, y_ms = float(np.median(t_kernel)), float(np.median(t_torch))
            entry["folded" if fold else "unfolded"] = dict(
                kernel_ms=t_kernel, torch_ms=t_torch, kernel_ms_per_sounding=k_ms / B, torch_ms_per_sounding=y_ms / Bt,
                ratio_torch_over_kernel=(y_ms / Bt) / (k_ms / B), counts_equal=equal)
            print("n_keep %5d %s: kernel %.3f ms / %d soundings, torch %.3f ms / %d soundings, per sounding x%.2f; counts equal: %s"
                  % (n_keep, "folded  " if fold else "unfolded", k_ms, B, y_ms, Bt, (y_ms / Bt) / (k_ms / B), equal))
            del want
        del less, leq, order, part
        torch.cuda.empty_cache()
        # the whole pipeline beside the diagnostics of the mean, on the same ensemble
        for fn in (ensembles.diagnostics, ensembles.rank_diagnostics):
            fn(ens, depth_edges, max_lag=MAX_LAG)
        torch.cuda.synchronize(dev)
        t_diag, t_rank = [], []
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        for _ in range(max(1, a.rounds // 2)):
            t_diag.append(events_ms(lambda: ensembles.diagnostics(ens, depth_edges, max_lag=MAX_LAG), dev)[0])
            t_rank.append(events_ms(lambda: ensembles.rank_diagnostics(ens, depth_edges, max_lag=MAX_LAG), dev)[0])
        entry["pipeline"] = dict(diagnostics_ms=t_diag, rank_diagnostics_ms=t_rank, ratio_rank_over_diagnostics=float(np.median(t_rank) / np.median(t_diag)),
                                 block_soundings=ensembles._rank_block(None, B, n_keep, N_DEPTH),
                                 peak_device_bytes_above_the_ensemble=int(torch.cuda.max_memory_allocated(dev) - base))
        print("n_keep %5d pipeline: diagnostics %.1f ms, rank_diagnostics %.1f ms (x%.2f), blocks of %d soundings, peak %.2f GiB"
              % (n_keep, np.median(t_diag), np.median(t_rank), entry["pipeline"]["ratio_rank_over_diagnostics"], entry["pipeline"]["block_soundings"],
                 entry["pipeline"]["peak_device_bytes_above_the_ensemble"] / 2.0 ** 30))
        result["sizes"][str(n_keep)] = entry
        del ens
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({n: {"unfolded": v["unfolded"]["ratio_torch_over_kernel"], "folded": v["folded"]["ratio_torch_over_kernel"]} for n, v in result["sizes"].items()}))
    return result


if __name__ == "__main__":
    main()
