"""What the posterior ensemble costs and what its two kernels deliver (DeviceChains(hitmap=True, ensemble=...); geobipy_amd.ensembles).

    python scripts/bench_ensembles.py kernels [--out profiles/ensembles/kernels.json]
    python scripts/bench_ensembles.py sampler --parent-lib scripts/ab/parent.so [--out profiles/ensembles/bench.json]

kernels   one process, device events, medians after warm-up, on a synthetic ensemble of 8 192 chains x 64 slots (K = 30) and 440 depth
          cells: the raster through its C entry on preallocated buffers, alternating with the torch formulation (a padded
          ``searchsorted`` plus ``gather`` on preallocated buffers too); output bytes over time against the ~6.3 TB/s the device
          streams; and the re-binning kernel beside one k_hitmap_classes<1> read of maps of the same size.
          The bar: the raster kernel is faster than the torch formulation.
sampler   as scripts/bench_data_posteriors.py: BASELINE config 5's block (8 192 chains, the driver gbp_rj_run chooses) and the
          1 024-chain persistent block, 2 000 iterations after 200 of warm-up, host clock around the synchronised run; six variants, each
          in a process of its own, run alternating and twice in one call:
    parent    the parent commit's library (--parent-lib: built beforehand, e.g. into scripts/ab/), no posteriors beyond bench.py's
    off       this tree's library, the same configuration: what bench.py measures
    hitmap    this tree's library with the hit map -- what the ensemble needs anyway
    data      ... plus the data-space posteriors and no ensemble: another "sampled extra", so the same instantiations of the accept /
              step / flush kernels run as with the ensemble -- what those cost before the ensemble adds anything
    ensemble  ... plus the ensemble at n_keep = 256 and the default thin of a 100 000-sample chain (391)
    thin1     ... plus the ensemble at n_keep = 256, thin = 1: every settle of the first 256 samples writes, then none does
          No figure is fixed beforehand.  The structs only grew at their ends, so the parent's library runs under this tree's Python
          with the feature off."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(solve_gradient=True, maximum_number_of_layers=30, minimum_depth=1.0, maximum_depth=150.0, minimum_thickness=1.0,
            initial_relative_error=0.05, minimum_relative_error=0.001, maximum_relative_error=0.5, initial_additive_error=5.0,
            minimum_additive_error=3.0, maximum_additive_error=20.0, relative_error_proposal_variance=1e-6,
            additive_error_proposal_variance=1e-6, probability_of_birth=1.0 / 6.0, probability_of_death=1.0 / 6.0,
            probability_of_perturb=1.0 / 6.0, probability_of_no_change=0.5)
BLOCKS = (("config5_8192", 8192, 0), ("persistent_1024", 1024, 2))
VARIANTS = {"off": {}, "hitmap": dict(hitmap=True), "data": dict(hitmap=True, data_posteriors=True), "ensemble": dict(hitmap=True, ensemble=dict(n_keep=256, thin=391)),
            "thin1": dict(hitmap=True, ensemble=dict(n_keep=256, thin=1))}
STREAM_TB_S = 6.3


def kernels(B, n_keep, K, n_depth, n_value, rounds, warm):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from geobipy_amd import _lib, ensembles, hitmap
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    width = 0.5
    k = torch.randint(1, K + 1, (B, n_keep), generator=g, device=dev, dtype=torch.int32)
    col = torch.arange(K, device=dev)[None, None, :]
    edges = torch.sort(torch.rand((B, n_keep, K), generator=g, device=dev, dtype=torch.float64) * (n_depth * width), dim=2).values
    edges = torch.where(col < k[:, :, None] - 1, edges, torch.full((), float("inf"), dtype=torch.float64, device=dev)).contiguous()
    edges = torch.sort(edges, dim=2).values.contiguous()
    sigma = torch.exp(torch.randn((B, n_keep, K), generator=g, device=dev, dtype=torch.float64) - 3.0)
    sigma = torch.where(col < k[:, :, None], sigma, torch.full((), float("nan"), dtype=torch.float64, device=dev)).contiguous()
    lmp = torch.full((B,), -3.0, dtype=torch.float64, device=dev)
    z = (torch.arange(n_depth, device=dev, dtype=torch.float64) + 0.5) * width
    slots = torch.arange(n_keep, device=dev, dtype=torch.int32)
    out = torch.empty((B, n_keep, n_depth), dtype=torch.float64, device=dev)
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream

    def raster():
        _lib.check(lib.gbp_ensemble_raster(B, n_keep, K, k.data_ptr(), edges.data_ptr(), sigma.data_ptr(), n_keep, slots.data_ptr(), n_depth,
                                           z.data_ptr(), out.data_ptr(), st))
    zz = z.expand(B, n_keep, n_depth).contiguous()
    idx = torch.empty((B, n_keep, n_depth), dtype=torch.int64, device=dev)
    out_t = torch.empty_like(out)
    sig0 = torch.nan_to_num(sigma, nan=0.0)

    def formulation():                       # (every slot filled here, so the formulation needs no NaN rows)
        torch.searchsorted(edges, zz, right=True, out=idx)
        torch.gather(sig0, 2, idx, out=out_t)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    raster(); formulation()
    torch.cuda.synchronize()
    assert torch.equal(out, out_t), "the raster kernel and the torch formulation disagree"
    t = {"raster": [], "torch": []}
    for r in range(warm + rounds):           # alternating in one process
        for name, fn in (("raster", raster), ("torch", formulation)):
            dt = timed(fn)
            if r >= warm:
                t[name].append(dt)
    del zz, idx, out_t, sig0
    res = {"shape": dict(chains=B, slots=n_keep, cells=n_depth, K=K), "rounds": rounds, "warmup": warm}
    nbytes = out.numel() * 8
    for name in t:
        res[name + "_s"] = dict(median=statistics.median(t[name]), min=min(t[name]))
    res["raster_output_TB_s"] = nbytes / res["raster_s"]["median"] * 1e-12
    res["raster_share_of_stream_rate"] = res["raster_output_TB_s"] / STREAM_TB_S
    res["raster_faster_than_torch"] = res["raster_s"]["median"] < res["torch_s"]["median"]
    res["torch_over_raster"] = res["torch_s"]["median"] / res["raster_s"]["median"]
    del out
    # the re-binning kernel beside one k_hitmap_classes<1> read of maps of the same size
    ens = ensembles.Ensemble(k, edges, sigma, torch.zeros((B, n_keep), dtype=torch.float64, device=dev), (k > 0).sum(dim=1), 1, lmp)
    hw = 4.0 * float(np.log(11.0) / np.log(10.0))
    maps = ensembles.rebin(ens, n_value, hw, (n_depth, width))["hitmap"]
    assert int(maps.sum()) == B * n_keep * n_depth
    tr, tc = [], []
    for r in range(warm + rounds):
        a = timed(lambda: ensembles.rebin(ens, n_value, hw, (n_depth, width)))
        b = timed(lambda: hitmap.class_probability(maps, lmp, hw, [0.0], [1.0]))
        if r >= warm:
            tr.append(a); tc.append(b)
    res["rebin_s"] = dict(median=statistics.median(tr), min=min(tr))
    res["classes1_read_s"] = dict(median=statistics.median(tc), min=min(tc))
    res["maps"] = dict(n_value=n_value, n_depth=n_depth, bytes=maps.numel() * 4)
    return res


def child(variant, lib, n_it, warm):
    sys.path.insert(0, ROOT)
    import torch
    from geobipy_amd import _lib
    if lib:
        _lib.LIB_PATH = os.path.abspath(lib)
        for name in ("gbp_ensemble_raster", "gbp_ensemble_rebin"):      # (entries the parent's library does not have)
            _lib.SIGNATURES.pop(name, None)
    from geobipy_amd import DeviceChains, FdemBatch, synthetic
    system = synthetic.syn10_system()
    kw = VARIANTS.get(variant, {})
    out = {}
    for name, B, mode in BLOCKS:
        nl, sig, thk, h = synthetic.draw_models(B, 4, seed=synthetic.SEED + 5)
        data = synthetic.noisy_observations(FdemBatch(system, nl, sig, thk, h, waves=2).forward().cpu().numpy())
        dc = DeviceChains(system, h, data, seed=1, exact_jacobian=False, **kw, **OPTS)
        dc.run_mode = mode
        dc.run(warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dc.run(n_it)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = B * n_it / dt
        out[name + "_accepted"] = int(dc.n_accepted.sum())
        if "ensemble" in kw:                                     # (every sample of every chain was seen once)
            out[name + "_seen"] = int(dc.ens_seen.sum())
            out[name + "_filled"] = int((dc.ens_k > 0).sum())
        del dc
    print("RESULT " + json.dumps(out), flush=True)


def sampler(a):
    variants = [("parent", a.parent_lib)] if a.parent_lib else []
    variants += [(v, None) for v in VARIANTS]
    runs = {v: [] for v, _ in variants}
    for rep in range(2):
        for v, lib in variants:                                  # alternating: every variant once, then every variant again
            cmd = [sys.executable, os.path.abspath(__file__), "child", "--variant", v, "--iterations", str(a.iterations), "--warmup", str(a.warmup)]
            if lib:
                cmd += ["--lib", lib]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stdout.write(p.stdout)
                raise SystemExit("variant %s failed (exit status %d): nothing further is started" % (v, p.returncode))
            runs[v].append(json.loads(line[0][7:]))
            print(v, rep, runs[v][-1], flush=True)
    res = {"unit": "chain-iterations/s", "iterations": a.iterations, "warmup": a.warmup, "runs": runs, "summary": {}}
    for name, B, _ in BLOCKS:
        s = {v: [r[name] for r in runs[v]] for v in runs}
        mean = {v: sum(x) / len(x) for v, x in s.items()}
        row = {"runs": s, "mean": mean, "ensemble_vs_hitmap": mean["ensemble"] / mean["hitmap"] - 1.0,
               "thin1_vs_hitmap": mean["thin1"] / mean["hitmap"] - 1.0, "data_vs_hitmap": mean["data"] / mean["hitmap"] - 1.0,
               "ensemble_vs_data": mean["ensemble"] / mean["data"] - 1.0,
               "same_chains_in_every_variant": len({r[name + "_accepted"] for v in VARIANTS for r in runs[v]}) == 1}
        if "parent" in s:
            row["parent_spread"] = abs(s["parent"][0] - s["parent"][1]) / mean["parent"]
            row["off_vs_parent"] = mean["off"] / mean["parent"] - 1.0
            row["same_chains_as_parent"] = {r[name + "_accepted"] for r in runs["parent"]} == {r[name + "_accepted"] for r in runs["off"]}
        res["summary"][name] = row
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernels", "sampler", "child"))
    ap.add_argument("--parent-lib", help="the parent commit's libgeobipy_amd.so")
    ap.add_argument("--out", default=None, help="write the JSON here too")
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--cells", type=int, default=440)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.what == "child":
        return child(a.variant, a.lib, a.iterations, a.warmup)
    res = kernels(a.chains, a.slots, 30, a.cells, 250, a.rounds, 3) if a.what == "kernels" else sampler(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
