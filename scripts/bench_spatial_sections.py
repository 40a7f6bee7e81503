"""Sections across flight lines (gbp_section_propagate): what a sweep of message passing costs on a survey.

A synthetic survey of 40 lines 150 m apart with 250 soundings 25 m apart each, n = 64 three-layer models per sounding: the first
interface follows a smooth surface under all lines with 2 m of jitter, and in 30 % of the soundings 40 of the 64 models belong to a decoy
family 15 m above or below it, the sign drawn per sounding.  The graph is ``sections.neighbours`` with max_distance = 1.5 line spacings,
the distances are ``sections.edge_distance``.

The C entry is timed on preallocated buffers between device events, medians after warm-up rounds, with 1 and with 1 + SWEEPS sweeps
taking turns in one process: seconds per sweep is the difference over SWEEPS, and what is left of the one-sweep call is the prepare
kernel (d2 -> K, one exp per entry) with the launches that run once (first messages, residuals, beliefs: S n and E n numbers, against
E n^2).  Beside them stands the floor of either, E n^2 8 B over the HBM bandwidth: a sweep reads K once, the prepare kernel reads d2 and
writes K (two floors).  The sweep count at which the residual passes 1e-6 is read off one long call.  There is no pass / fail
threshold: nobody has measured this before, the numbers go into DESIGN.md 3.28.  Writes one JSON file.

    python scripts/bench_spatial_sections.py [--lines 40] [--soundings 250] [--models 64] [--rounds 7] [--warmup 2] [--sweeps 32]
                                             [--seed 0] [--out profiles/spatial_sections/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from geobipy_amd import _lib, sections      # noqa: E402
from geobipy_amd.ensembles import Ensemble      # noqa: E402

Z1, ALONG, ACROSS = 120.0, 25.0, 150.0
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12                                       # B/s: the specification, and what a streaming copy reaches


def synthetic_survey(lines, per_line, n, seed):
    """(k [S, n], edges, sigma [S, n, 4], x, y, ptr) in numpy."""
    rng = np.random.default_rng(seed)
    S, K = lines * per_line, 4
    x, y = np.tile(ALONG * np.arange(per_line), lines), np.repeat(ACROSS * np.arange(lines), per_line)
    truth = 30.0 + 10.0 * np.sin(x / 150.0) + 5.0 * np.cos(y / 400.0)
    top = truth[:, None] + rng.normal(0.0, 2.0, (S, n))
    decoy = rng.uniform(size=S) < 0.3
    top[:, :(5 * n) // 8] += np.where(decoy, rng.choice([-15.0, 15.0], S), 0.0)[:, None]
    k = np.full((S, n), 3, dtype=np.int32)
    edges, sigma = np.full((S, n, K), np.inf), np.full((S, n, K), np.nan)
    edges[:, :, 0], edges[:, :, 1] = top, 80.0 + rng.normal(0.0, 2.0, (S, n))
    sigma[:, :, :3] = 10.0 ** (np.array([-2.0, -0.5, -1.5]) + rng.normal(0.0, 0.05, (S, n, 3)))
    return k, edges, sigma, x, y, np.arange(lines + 1, dtype=np.int64) * per_line


def events_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--lines", type=int, default=40)
    p.add_argument("--soundings", type=int, default=250, help="per line")
    p.add_argument("--models", type=int, default=64)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sweeps", type=int, default=32, help="the sweeps the per-sweep time is taken over")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "spatial_sections", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spatial_sections needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    n = a.models
    k, edges, sigma, x, y, ptr = synthetic_survey(a.lines, a.soundings, n, a.seed)
    S = k.shape[0]
    ens = Ensemble(torch.as_tensor(k).to(dev), torch.as_tensor(edges).to(dev), torch.as_tensor(sigma).to(dev), None, None, 1, None)
    rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(S, n).contiguous()
    eu, ev, g, dist = sections.neighbours(x, y, ptr, None, max_distance=1.5 * ACROSS)
    E = int(eu.size)
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count,
                  lines=a.lines, soundings_per_line=a.soundings, soundings=S, models=n, edges=E, edges_across_lines=int(np.sum(ev != eu + 1)),
                  max_degree=int(np.bincount(np.concatenate([eu, ev])).max()), spacing_m=[ALONG, ACROSS], max_distance_m=1.5 * ACROSS,
                  rounds=a.rounds, warmup=a.warmup, sweeps_timed=a.sweeps)
    d2 = sections.edge_distance(ens, rows, eu, ev, 0.0, Z1)
    long = sections.propagate(d2, g, eu, ev, np.full(S, n), S, sweeps=1024)
    residual = long["residual"].cpu().numpy()
    below = np.flatnonzero(residual < 1e-6)
    result.update(residual_at_sweeps={str(t): float(residual[t - 1]) for t in (1, 2, 5, 10, 20, 32, 50, 100, 200, 300, 500, 1024)},
                  sweeps_to_residual_1e_6=int(below[0]) + 1 if below.size else None, beliefs_finite=bool(torch.isfinite(long["belief"]).all()))
    del long
    in_ptr, in_edge = sections.incoming(eu, ev, S)
    i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(dev)      # noqa: E731
    t_eu, t_ev, t_nu, t_ptr, t_edge = i32(eu), i32(ev), i32(np.full(S, n)), i32(in_ptr), i32(in_edge)
    f64 = dict(dtype=torch.float64, device=dev)
    most = 1 + a.sweeps
    t_g, score = torch.as_tensor(g).to(dev), torch.zeros((S, n), **f64)
    K, w, mu, resid = torch.empty_like(d2), torch.empty((S, n), **f64), torch.empty((2, 2 * E, n), **f64), torch.empty((most, 2 * E), **f64)
    belief, state, res = torch.empty((S, n), **f64), torch.empty(S, dtype=torch.int32, device=dev), torch.empty(most, **f64)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(sweeps):
        _lib.check(lib.gbp_section_propagate(S, E, n, t_eu.data_ptr(), t_ev.data_ptr(), t_nu.data_ptr(), score.data_ptr(), t_g.data_ptr(), d2.data_ptr(),
                                             t_ptr.data_ptr(), t_edge.data_ptr(), sweeps, 0.0, K.data_ptr(), w.data_ptr(), mu.data_ptr(), resid.data_ptr(),
                                             belief.data_ptr(), state.data_ptr(), res.data_ptr(), stream))

    t = {1: [], most: []}
    for r in range(a.warmup + a.rounds):
        for sweeps in (1, most):                                              # taking turns
            ms = events_ms(lambda: call(sweeps), dev)
            if r >= a.warmup:
                t[sweeps].append(ms)
    one, many = float(np.median(t[1])), float(np.median(t[most]))
    per_sweep = (many - one) / a.sweeps * 1e-3
    slab = E * n * n * 8
    result.update(ms_one_sweep_call=t[1], ms_many_sweep_call=t[most], seconds_per_sweep=per_sweep, seconds_prepare=one * 1e-3 - per_sweep,
                  seconds_prepare_note="the one-sweep call less one sweep: k_graph_kernel with the launches that run once (first messages, residuals, beliefs)",
                  bytes_K=slab, floor_seconds_per_sweep=dict(hbm_peak=slab / HBM_PEAK, hbm_achievable=slab / HBM_ACHIEVABLE),
                  floor_seconds_prepare=dict(hbm_peak=2 * slab / HBM_PEAK, hbm_achievable=2 * slab / HBM_ACHIEVABLE),
                  sweep_share_of_achievable_floor=(slab / HBM_ACHIEVABLE) / per_sweep if per_sweep > 0 else None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({name: result[name] for name in ("edges", "seconds_per_sweep", "seconds_prepare", "floor_seconds_per_sweep", "sweeps_to_residual_1e_6")}))
    return result


if __name__ == "__main__":
    main()
