"""The evidence of the lateral coupling along lines (gbp_section_evidence).

One launch of T = 8 rungs against what a user had to do before to scan tau: 8 calls of gbp_section_track with marginals on the same
d2, one per value of g.  The condition is that the evidence launch is not slower in the same run; the ratio is recorded, with the
largest distance between the launch's log_partition and the 8 calls' (the same quantity by two routes).  The T = 1 launch is recorded
beside the Viterbi launch of the same run, for reading: there is no bar on it.

64 sequences of 1 024 soundings 25 m apart, n = 128 models per sounding, K = 30: the shapes and the synthetic ensembles of
bench_sections.py.  The C entries are timed on preallocated buffers with device events, medians after warm-up rounds, taking turns in
one process.  Writes one JSON file.

    python scripts/bench_section_evidence.py [--sequences 64] [--soundings 1024] [--models 128] [--rounds 5] [--warmup 2]
                                             [--tau-max 0.8] [--out profiles/section_evidence/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_ensemble_correlation import K, events_ms, synthetic      # noqa: E402  (the ensembles bench_families.py times)
from bench_sections import SPACING, Z1      # noqa: E402
from geobipy_amd import _lib, sections      # noqa: E402

RUNGS = 8


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--soundings", type=int, default=1024, help="per sequence")
    p.add_argument("--models", type=int, default=128)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--tau-max", type=float, default=0.8, help="the ladder's first rung; tau falls by sqrt 2 per rung")
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "section_evidence", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_section_evidence needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    L, N, n = a.sequences, a.soundings, a.models
    S = L * N
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count,
                  sequences=L, soundings_per_sequence=N, models=n, K=K, z1=Z1, spacing_m=SPACING, rounds=a.rounds, warmup=a.warmup, rungs=RUNGS,
                  tau_max=a.tau_max)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ens = synthetic(S, n, dev, seed=n)
    rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(S, n).contiguous()
    n_used = torch.full((S,), n, dtype=torch.int32, device=dev)
    ptr_h = np.arange(L + 1, dtype=np.int64) * N
    ptr = torch.as_tensor(ptr_h).to(dev)
    partner = torch.as_tensor(sections.partners(ptr_h, np.full(S, n))).to(dev)
    x = np.tile(SPACING * np.arange(N), L)
    g_h = sections.steps(x, np.zeros(S), tau=a.tau_max, ptr=ptr_h)
    g = [torch.as_tensor(g_h * 2.0 ** t).to(dev) for t in range(RUNGS)]       # rung t as a caller of gbp_section_track has to pass it
    d2 = torch.empty((S, n, n), dtype=torch.float64, device=dev)
    _lib.check(lib.gbp_ensemble_cross_distance(S, n, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), n, rows.data_ptr(),
                                               partner.data_ptr(), 0.0, Z1, 0, 1, 1, d2.data_ptr(), stream))
    score = torch.zeros((S, n), dtype=torch.float64, device=dev)
    back = torch.empty((S, n), dtype=torch.int16, device=dev)
    state = torch.empty((S,), dtype=torch.int32, device=dev)
    log_score = torch.empty((L,), dtype=torch.float64, device=dev)
    scan_lp = torch.empty((RUNGS, L), dtype=torch.float64, device=dev)
    marginal, scale = torch.empty((S, n), dtype=torch.float64, device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
    lz, dlz = (torch.empty((RUNGS, L), dtype=torch.float64, device=dev) for _ in range(2))
    lz1, dlz1 = (torch.empty((1, L), dtype=torch.float64, device=dev) for _ in range(2))

    def track(t, with_marginals):
        m = (marginal.data_ptr(), scan_lp[t].data_ptr(), scale.data_ptr()) if with_marginals else (None, None, None)
        _lib.check(lib.gbp_section_track(L, ptr.data_ptr(), S, n, n_used.data_ptr(), score.data_ptr(), g[t].data_ptr(), d2.data_ptr(), back.data_ptr(),
                                         state.data_ptr(), log_score.data_ptr(), m[0], m[1], m[2], stream))

    def scan():
        for t in range(RUNGS):
            track(t, True)

    def evidence(T, out, dout):
        _lib.check(lib.gbp_section_evidence(L, ptr.data_ptr(), S, n, n_used.data_ptr(), score.data_ptr(), g[0].data_ptr(), d2.data_ptr(), T,
                                            out.data_ptr(), dout.data_ptr(), stream))

    turns = (("evidence_8", lambda: evidence(RUNGS, lz, dlz)), ("scan_8_tracks_with_marginals", scan), ("evidence_1", lambda: evidence(1, lz1, dlz1)),
             ("viterbi", lambda: track(0, False)))
    for _ in range(a.warmup):
        for _, fn in turns:
            fn()
    torch.cuda.synchronize(dev)
    t = {name: [] for name, _ in turns}
    for _ in range(a.rounds):
        for name, fn in turns:
            t[name].append(events_ms(fn, dev)[0])
    med = {name: float(np.median(v)) for name, v in t.items()}
    finite = bool(torch.isfinite(lz).all() and torch.isfinite(dlz).all() and torch.isfinite(scan_lp).all())
    f = (dlz.sum(dim=1) + 0.5 * (S - L)).cpu().numpy()
    result["evidence"] = dict(evidence_8_ms=t["evidence_8"], scan_8_tracks_with_marginals_ms=t["scan_8_tracks_with_marginals"], evidence_1_ms=t["evidence_1"],
                              viterbi_ms=t["viterbi"], ratio_scan_over_evidence=med["scan_8_tracks_with_marginals"] / med["evidence_8"],
                              evidence_no_slower=bool(med["evidence_8"] <= med["scan_8_tracks_with_marginals"]), all_finite=finite,
                              largest_log_partition_distance=float((lz - scan_lp).abs().max()), largest_log_partition=float(scan_lp.abs().max()),
                              first_rung_equals_single_rung_launch=bool(torch.equal(lz[:1], lz1) and torch.equal(dlz[:1], dlz1)),
                              tau_ladder=(a.tau_max / np.sqrt(2.0 ** np.arange(RUNGS))).tolist(), evidence_derivative=f.tolist(),
                              d2_bytes_per_s_evidence_8=float(S - L) * n * n * 8 / (med["evidence_8"] * 1e-3),
                              d2_bytes_per_s_evidence_1=float(S - L) * n * n * 8 / (med["evidence_1"] * 1e-3))
    result["condition_met"] = bool(result["evidence"]["evidence_no_slower"] and finite)
    print("evidence, 8 rungs %.3f ms; 8 tracks with marginals %.3f ms (x%.2f); 1 rung %.3f ms beside viterbi %.3f ms; largest distance of log Z %.3g"
          % (med["evidence_8"], med["scan_8_tracks_with_marginals"], result["evidence"]["ratio_scan_over_evidence"], med["evidence_1"], med["viterbi"],
             result["evidence"]["largest_log_partition_distance"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(condition_met=result["condition_met"], ratio_scan_over_evidence=result["evidence"]["ratio_scan_over_evidence"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
