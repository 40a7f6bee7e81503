"""Sections of sampled models along lines (gbp_ensemble_cross_distance and gbp_section_track).

The chain against the loop a user would write in torch over the same d2, batched over the sequences: per step
``(V[:, :, None] - g * d2).max(1)``, the back-pointers kept, then the walk back with one gather per step.  Every operation of that
loop is one fp64 multiply, subtract or compare, as in the kernel, so the two paths must be ``torch.equal``; the condition is that they
are and that the kernel is no slower than the loop in the same run.  The script records what it measured and whether the condition
holds.  The forward-backward launch has no yardstick: its time is recorded.

The cross distance needs no speed: its time is listed beside gbp_ensemble_distance's pairs per second on the same ensemble.

64 sequences of 1 024 soundings 25 m apart, n = 128 models per sounding, K = 30, the synthetic ensembles of bench_families.py.  The C
entries are timed on preallocated buffers with device events, medians after warm-up rounds, taking turns with the yardstick in one
process.  Writes one JSON file.

``--draws R`` also times gbp_section_draw on the same d2: the filter launch and the draw launch of R joint realisations
per sequence together, between device events, beside the chain's times of the same run.  It has no yardstick either: the time is
recorded, with the share of draws that fall on the Viterbi path and the spread of the smoothed marginals they reproduce.

    python scripts/bench_sections.py [--sequences 64] [--soundings 1024] [--models 128] [--rounds 5] [--draws 0] [--seed 0]
                                     [--out profiles/sections/bench.json]
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
from geobipy_amd import _lib, families, sections      # noqa: E402

Z1, SPACING = 165.0, 25.0


def torch_viterbi(d2, g, L, N, n):
    """(state int32 [L * N], log_score [L]) of L sequences of N soundings with n models each, equal weights: the loop in torch."""
    dv, gv = d2.view(L, N, n, n), g.view(L, N)
    V = torch.zeros((L, n), dtype=torch.float64, device=d2.device)
    back = torch.empty((N, L, n), dtype=torch.int64, device=d2.device)
    for r in range(N - 1):
        V, back[r + 1] = (V[:, :, None] - gv[:, r, None, None] * dv[:, r]).max(1)
    top, cur = V.max(1)
    state = torch.empty((L, N), dtype=torch.int64, device=d2.device)
    for r in range(N - 1, -1, -1):
        state[:, r] = cur
        if r > 0:
            cur = torch.gather(back[r], 1, cur[:, None])[:, 0]
    return state.reshape(-1).to(torch.int32), top


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--soundings", type=int, default=1024, help="per sequence")
    p.add_argument("--models", type=int, default=128)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--draws", type=int, default=0, help="joint realisations per sequence to draw and time (0: none)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "sections", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sections needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    L, N, n = a.sequences, a.soundings, a.models
    S = L * N
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count,
                  sequences=L, soundings_per_sequence=N, models=n, K=K, z1=Z1, spacing_m=SPACING, rounds=a.rounds, warmup=a.warmup)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ens = synthetic(S, n, dev, seed=n)
    rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(S, n).contiguous()
    n_used = torch.full((S,), n, dtype=torch.int32, device=dev)
    ptr_h = np.arange(L + 1, dtype=np.int64) * N
    ptr = torch.as_tensor(ptr_h).to(dev)
    partner = torch.as_tensor(sections.partners(ptr_h, np.full(S, n))).to(dev)
    x = np.tile(SPACING * np.arange(N), L)
    g = torch.as_tensor(sections.steps(x, np.zeros(S), ptr=ptr_h)).to(dev)
    d2 = torch.empty((S, n, n), dtype=torch.float64, device=dev)
    score = torch.zeros((S, n), dtype=torch.float64, device=dev)
    back = torch.empty((S, n), dtype=torch.int16, device=dev)
    state = torch.empty((S,), dtype=torch.int32, device=dev)
    log_score, log_partition = (torch.empty((L,), dtype=torch.float64, device=dev) for _ in range(2))
    marginal, scale = torch.empty((S, n), dtype=torch.float64, device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
    step = max(1, families.DISTANCE_BLOCK_BYTES // (n * n * 8))          # soundings per launch, as families.distance blocks them

    def distance():
        for b0 in range(0, S, step):
            nb = min(S, b0 + step) - b0
            _lib.check(lib.gbp_ensemble_distance(nb, n, K, ens.k[b0:].data_ptr(), ens.edges[b0:].data_ptr(), ens.sigma[b0:].data_ptr(), n,
                                                 rows[b0:].data_ptr(), 0.0, Z1, 0, 1, 1, d2[b0:].data_ptr(), stream))

    def cross():
        _lib.check(lib.gbp_ensemble_cross_distance(S, n, K, ens.k.data_ptr(), ens.edges.data_ptr(), ens.sigma.data_ptr(), n, rows.data_ptr(),
                                                   partner.data_ptr(), 0.0, Z1, 0, 1, 1, d2.data_ptr(), stream))

    def track(with_marginals):
        m = (marginal.data_ptr(), log_partition.data_ptr(), scale.data_ptr()) if with_marginals else (None, None, None)
        _lib.check(lib.gbp_section_track(L, ptr.data_ptr(), S, n, n_used.data_ptr(), score.data_ptr(), g.data_ptr(), d2.data_ptr(), back.data_ptr(),
                                         state.data_ptr(), log_score.data_ptr(), m[0], m[1], m[2], stream))

    # ---- the two distance entries, the within-sounding one first: the cross distances stay in d2 for the chain
    t = dict(distance=[], cross=[])
    for name, fn in (("distance", distance), ("cross", cross)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        for _ in range(a.rounds):
            t[name].append(events_ms(fn, dev)[0])
    med_d, med_c = float(np.median(t["distance"])), float(np.median(t["cross"]))
    result["distance"] = dict(distance_ms=t["distance"], cross_distance_ms=t["cross"], distance_pairs_per_s=S * n * (n - 1) / 2.0 / (med_d * 1e-3),
                              cross_distance_pairs_per_s=float(S - L) * n * n / (med_c * 1e-3), bytes=float(S) * n * n * 8,
                              largest_squared_distance=float(torch.nan_to_num(d2, nan=0.0).max()))
    print("distance %.3f ms (%.3g pairs/s); cross distance %.3f ms (%.3g pairs/s); %.2f GB each"
          % (med_d, result["distance"]["distance_pairs_per_s"], med_c, result["distance"]["cross_distance_pairs_per_s"], S * n * n * 8 / 1e9))

    # ---- the chain, taking turns with the loop in torch
    for _ in range(a.warmup):
        track(False)
        track(True)
        torch_viterbi(d2, g, L, N, n)
    torch.cuda.synchronize(dev)
    t = dict(viterbi=[], both=[], torch=[])
    for _ in range(a.rounds):
        t["viterbi"].append(events_ms(lambda: track(False), dev)[0])
        ms, (want_state, want_top) = events_ms(lambda: torch_viterbi(d2, g, L, N, n), dev)
        t["torch"].append(ms)
        t["both"].append(events_ms(lambda: track(True), dev)[0])
    med = {name: float(np.median(v)) for name, v in t.items()}
    same = bool(torch.equal(state, want_state)) and bool(torch.equal(log_score, want_top))
    weights = marginal.sum(dim=1)
    result["chain"] = dict(viterbi_ms=t["viterbi"], viterbi_and_marginals_ms=t["both"], torch_loop_ms=t["torch"], ratio_torch_over_kernel=med["torch"] / med["viterbi"],
                           paths_equal=same, kernel_no_slower=bool(med["viterbi"] <= med["torch"]), condition_met=bool(same and med["viterbi"] <= med["torch"]),
                           d2_bytes_per_s_viterbi=float(S - L) * n * n * 8 / (med["viterbi"] * 1e-3), marginals_finite=bool(torch.isfinite(marginal).all()),
                           largest_row_sum_error=float((weights - 1.0).abs().max()), mean_n_effective=float((1.0 / (marginal * marginal).sum(dim=1)).mean()))
    print("chain: viterbi %.3f ms; torch loop %.3f ms (x%.2f); paths equal: %s; with marginals %.3f ms"
          % (med["viterbi"], med["torch"], result["chain"]["ratio_torch_over_kernel"], same, med["both"]))
    if a.draws > 0:
        R = a.draws
        filtered, scale_ws = torch.empty((S, n), dtype=torch.float64, device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
        draw_state = torch.empty((R, S), dtype=torch.int32, device=dev)

        def draw():
            _lib.check(lib.gbp_section_draw(L, ptr.data_ptr(), S, n, n_used.data_ptr(), score.data_ptr(), g.data_ptr(), d2.data_ptr(), None, a.seed, R,
                                            filtered.data_ptr(), scale_ws.data_ptr(), draw_state.data_ptr(), stream))

        for _ in range(a.warmup):
            draw()
        torch.cuda.synchronize(dev)
        t_draw = [events_ms(draw, dev)[0] for _ in range(a.rounds)]
        med_draw = float(np.median(t_draw))
        track(True)                                                         # the smoothed marginals of the same chain, for the draws' frequencies
        torch.cuda.synchronize(dev)
        freq = torch.zeros((S, n), dtype=torch.float64, device=dev)
        freq.scatter_add_(1, draw_state.long().t().contiguous(), torch.ones((S, R), dtype=torch.float64, device=dev))
        z = ((freq - R * marginal) / torch.sqrt((R * marginal * (1.0 - marginal)).clamp(min=1e-300)))[R * marginal >= 5.0]
        result["draws"] = dict(n_draws=R, seed=a.seed, filter_and_draw_ms=t_draw, viterbi_and_marginals_ms_median=med["both"], viterbi_ms_median=med["viterbi"],
                               sounding_draws_per_s=float(R) * S / (med_draw * 1e-3), states_in_range=bool(((draw_state >= 0) & (draw_state < n)).all()),
                               share_of_sounding_draws_on_the_viterbi_path=float((draw_state == state[None, :]).double().mean()),
                               cells_compared=int(z.numel()), rms_z_against_the_marginals=float(torch.sqrt((z * z).mean())) if z.numel() else None)
        print("draws: filter + %d draws per sequence %.3f ms (%.3g sounding-draws/s); rms z against the marginals %.3f over %d cells"
              % (R, med_draw, result["draws"]["sounding_draws_per_s"], result["draws"]["rms_z_against_the_marginals"] or 0.0, z.numel()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(condition_met=result["chain"]["condition_met"], ratio_torch_over_kernel=result["chain"]["ratio_torch_over_kernel"],
                          cross_distance_pairs_per_s=result["distance"]["cross_distance_pairs_per_s"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
