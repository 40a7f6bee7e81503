"""Model families of an ensemble (gbp_ensemble_distance and gbp_distance_families).

The distance kernel against the same quantity as a user would otherwise write it in torch: ensembles.realisations on 440 depth cells
-> torch.cdist -> / sqrt(440).  That is an APPROXIMATION of the integral the kernel evaluates exactly (a cell that holds an interface
takes one side's value), so the largest difference between the two is recorded beside the times, not held to a bound.  The clustering
kernel has no yardstick: its time per sounding and per stage is recorded.

The synthetic ensembles of bench_ensemble_correlation.py: B soundings, K = 30, 256 and 1 024 kept models, the window 0 .. 165 m.  The C
entries are timed on preallocated buffers with device events, medians after warm-up rounds; the yardstick runs in the same process,
taking turns with the kernel, on as many soundings as fit the device, and is compared per sounding.  No speed is required: the script
records what it measured.  Writes one JSON file.

    python scripts/bench_families.py [--soundings 1024] [--rounds 5] [--out profiles/families/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_ensemble_correlation import K, N_DEPTH, events_ms, synthetic      # noqa: E402  (the ensembles that script times)
from geobipy_amd import _lib, ensembles, families      # noqa: E402

Z1, Q_MAX, MAX_ITER = 165.0, 4, 100


def yardstick(ens, depth_edges):
    """D [B, n, n] from the series written out on the depth axis: the RMS difference over the cells."""
    x = ensembles.realisations(ens, depth_edges)                         # [B, n, V], log10
    return torch.cdist(x, x) / float(x.shape[2]) ** 0.5


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--soundings", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "families", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_families needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    B = a.soundings
    depth_edges = np.arange(N_DEPTH + 1) * (Z1 / N_DEPTH)
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count,
                  soundings=B, K=K, n_depth=N_DEPTH, z1=Z1, q_max=Q_MAX, max_iter=MAX_ITER, rounds=a.rounds, warmup=a.warmup, sizes={})
    stream = torch.cuda.current_stream(dev).cuda_stream
    for n in a.sizes:
        ens = synthetic(B, n, dev, seed=n)
        rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(B, n).contiguous()
        n_used = torch.full((B,), n, dtype=torch.int32, device=dev)
        D = torch.empty((B, n, n), dtype=torch.float64, device=dev)
        step = max(1, families.DISTANCE_BLOCK_BYTES // (n * n * 8))      # soundings per launch, as families.distance blocks them
        medoid = torch.empty((B, Q_MAX, Q_MAX), dtype=torch.int32, device=dev)
        label = torch.empty((B, Q_MAX, n), dtype=torch.int32, device=dev)
        nearest, second = (torch.empty((B, Q_MAX, n), dtype=torch.float64, device=dev) for _ in range(2))
        iterations, n_found = torch.empty((B, Q_MAX), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        converged = torch.empty((B, Q_MAX), dtype=torch.uint8, device=dev)

        def distance():
            for b0 in range(0, B, step):
                nb = min(B, b0 + step) - b0
                _lib.check(lib.gbp_ensemble_distance(nb, n, K, ens.k[b0:].data_ptr(), ens.edges[b0:].data_ptr(), ens.sigma[b0:].data_ptr(), n,
                                                     rows[b0:].data_ptr(), 0.0, Z1, 0, 1, 0, D[b0:].data_ptr(), stream))

        def cluster():
            _lib.check(lib.gbp_distance_families(B, n, D.data_ptr(), n_used.data_ptr(), Q_MAX, MAX_ITER, medoid.data_ptr(), label.data_ptr(),
                                                 nearest.data_ptr(), second.data_ptr(), iterations.data_ptr(), converged.data_ptr(),
                                                 n_found.data_ptr(), stream))
        # the yardstick's block: the series and its log10, and cdist's output with its scaled copy, twice (the last answer is kept)
        per = 8.0 * (4.0 * n * N_DEPTH + 4.0 * n * n)
        Bt = int(max(1, min(B, 0.5 * torch.cuda.mem_get_info(dev)[0] // per)))
        part = ensembles.Ensemble(ens.k[:Bt], ens.edges[:Bt], ens.sigma[:Bt], ens.misfit[:Bt], ens.count[:Bt], 1, ens.log_mean_prior[:Bt])
        for _ in range(a.warmup):
            distance()
            cluster()
            yardstick(part, depth_edges)
        torch.cuda.synchronize(dev)
        t = dict(distance=[], cluster=[], torch=[])
        for _ in range(a.rounds):                                        # taking turns, in one process
            t["distance"].append(events_ms(distance, dev)[0])
            ms, want = events_ms(lambda: yardstick(part, depth_edges), dev)
            t["torch"].append(ms)
            t["cluster"].append(events_ms(cluster, dev)[0])
        med = {name: float(np.median(v)) for name, v in t.items()}
        diff = float((D[:Bt] - want).abs().max())
        stages = int(n_found.sum())
        updates = int(iterations.sum())
        per_k, per_y = med["distance"] / B, med["torch"] / Bt
        entry = dict(distance_ms=t["distance"], cluster_ms=t["cluster"], torch_cdist_ms=t["torch"], torch_soundings=Bt,
                     distance_ms_per_sounding=per_k, torch_cdist_ms_per_sounding=per_y, ratio_torch_over_kernel=per_y / per_k,
                     pairs_per_s=B * n * (n - 1) / 2.0 / (med["distance"] * 1e-3), largest_difference_from_the_raster=diff,
                     largest_distance=float(D.max()), cluster_ms_per_sounding=med["cluster"] / B, stages_found=stages, updates=updates,
                     cluster_ms_per_sounding_and_stage=med["cluster"] / max(stages, 1), all_converged=bool(converged[n_found[:, None] > torch.arange(Q_MAX, device=dev)[None, :]].all()),
                     distance_bytes=float(B) * n * n * 8)
        result["sizes"][str(n)] = entry
        print("n %5d: distance %.3f ms / %d soundings; torch raster + cdist %.3f ms / %d soundings; per sounding x%.2f; largest difference %.3g of at most "
              "%.3g decades; clustering %.3f ms (%d stages, %d updates)" % (n, med["distance"], B, med["torch"], Bt, entry["ratio_torch_over_kernel"], diff,
                                                                            entry["largest_distance"], med["cluster"], stages, updates))
        del ens, part, want, D
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({n: {"ratio_torch_over_kernel": v["ratio_torch_over_kernel"], "cluster_ms_per_sounding": v["cluster_ms_per_sounding"]}
                      for n, v in result["sizes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
