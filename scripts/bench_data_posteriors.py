"""What the data-space posteriors cost the sampler (DeviceChains(hitmap=True, data_posteriors=True)).

    python scripts/bench_data_posteriors.py --parent-lib scripts/ab/parent.so [--out profiles/data_posteriors/bench.json]

Two blocks, 2 000 iterations after 200 of warm-up, host clock around the synchronised run: BASELINE config 5's block (8 192 chains, the
driver gbp_rj_run chooses) and the 1 024-chain block of its 8-GPU split (persistent kernel).  Four variants, each in a process of its
own, run alternating and twice in one call:
    parent    the parent commit's library (--parent-lib: built beforehand, e.g. into scripts/ab/), no posteriors beyond bench.py's
    off       this tree's library, the same configuration: what bench.py measures
    hitmap    this tree's library with the hit map -- what the data posteriors need anyway
    data      ... plus the data-space posteriors (64 cells, every channel's residual and the misfit)
The bar: off may be lower than parent by no more than the parent's own run-to-run spread (its two runs of this call).  data vs hitmap
is the feature's cost.  The structs only grew at their ends, so the parent's library runs under this tree's Python with the feature off."""
import argparse
import json
import os
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


def child(variant, lib, n_it, warm):
    sys.path.insert(0, ROOT)
    import torch
    from geobipy_amd import _lib
    if lib:
        _lib.LIB_PATH = os.path.abspath(lib)
    from geobipy_amd import DeviceChains, FdemBatch, synthetic
    system = synthetic.syn10_system()
    kw = {}
    if variant in ("hitmap", "data"):
        kw["hitmap"] = True
    if variant == "data":
        kw["data_posteriors"] = True
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
        if variant == "data":                                    # (every kept state of every chain was counted once)
            out[name + "_misfit_samples"] = int(dc.misfit_hist.sum())
        del dc
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="the parent commit's libgeobipy_amd.so")
    ap.add_argument("--out", default=None, help="write the JSON here too")
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib, a.iterations, a.warmup)
    variants = [("parent", a.parent_lib)] if a.parent_lib else []
    variants += [("off", None), ("hitmap", None), ("data", None)]
    runs = {v: [] for v, _ in variants}
    for rep in range(2):
        for v, lib in variants:                                  # alternating: every variant once, then every variant again
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--iterations", str(a.iterations), "--warmup", str(a.warmup)]
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
        row = {"runs": s, "mean": mean, "data_vs_hitmap": mean["data"] / mean["hitmap"] - 1.0,
               "same_chains_off_vs_hitmap_vs_data": len({r[name + "_accepted"] for v in ("off", "hitmap", "data") for r in runs[v]}) == 1}
        if "parent" in s:
            row["parent_spread"] = abs(s["parent"][0] - s["parent"][1]) / mean["parent"]
            row["off_vs_parent"] = mean["off"] / mean["parent"] - 1.0
            row["off_within_parent_spread"] = row["off_vs_parent"] >= -row["parent_spread"]
            row["same_chains_as_parent"] = {r[name + "_accepted"] for r in runs["parent"]} == {r[name + "_accepted"] for r in runs["off"]}
        res["summary"][name] = row
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
