"""The most probable section across flight lines (gbp_section_graph_path): what a max-sum sweep costs beside a
sum-product sweep of gbp_section_propagate, and what the level-by-level decode costs on a long line.

The survey is the synthetic one of bench_spatial_sections.py (40 lines 150 m apart, 250 soundings 25 m apart, n = 64 models, the graph
of ``sections.neighbours`` at 1.5 line spacings, the distances of ``sections.edge_distance``).  Both entries are timed on preallocated
buffers between device events, medians after warm-up rounds, with 1 and with 1 + SWEEPS sweeps taking turns in one process: seconds per
sweep is the difference over SWEEPS.  The two sweeps stream the same E n^2 8 bytes -- K there, d2 here -- so the sum-product sweep is
the yardstick, and E n^2 8 B over the HBM bandwidth the floor of either.  What is left of the one-sweep call of the path entry is the
launches that run once: the first messages, the residuals, the max-marginals and the decode, one launch per breadth-first level.

The decode is timed where it is longest: one line of --line soundings is a path graph with as many levels as soundings.  Its one-sweep
call less one sweep, over the levels, is the cost of a level: a launch of a single workgroup.  The refinement
(gbp_section_graph_refine) is timed on the survey per sweep over all colours, for one section.

There is no pass / fail threshold: nobody has measured this before, the numbers go into DESIGN.md 3.32.  Writes one JSON file.

    python scripts/bench_spatial_path.py [--lines 40] [--soundings 250] [--models 64] [--line 4000] [--rounds 7] [--warmup 2]
                                         [--sweeps 32] [--seed 0] [--out profiles/spatial_path/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_spatial_sections import ACROSS, HBM_ACHIEVABLE, HBM_PEAK, Z1, events_ms, synthetic_survey      # noqa: E402
from geobipy_amd import _lib, sections      # noqa: E402
from geobipy_amd.ensembles import Ensemble      # noqa: E402


def timed(call, sweeps, rounds, warmup, dev):
    """Medians (ms) of ``call(1)`` and ``call(1 + sweeps)``, taking turns, and the seconds per sweep between them."""
    most = 1 + sweeps
    t = {1: [], most: []}
    for r in range(warmup + rounds):
        for s in (1, most):
            ms = events_ms(lambda: call(s), dev)
            if r >= warmup:
                t[s].append(ms)
    one, many = float(np.median(t[1])), float(np.median(t[most]))
    return one, many, (many - one) / sweeps * 1e-3


class Graph:
    """The device buffers both entries take for one graph, and their calls."""

    def __init__(self, eu, ev, g, d2, S, n, most, dev):
        self.lib, self.dev, self.S, self.E, self.n = _lib.load(), dev, S, int(eu.size), n
        E = self.E
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(dev)      # noqa: E731
        f64 = dict(dtype=torch.float64, device=dev)
        in_ptr, in_edge = sections.incoming(eu, ev, S)
        self.level, self.level_ptr, level_node = sections.decode_levels(eu, ev, S)
        self.colour_ptr, colour_node = sections._colour_lists(eu, ev, S)
        self.t = dict(eu=i32(eu), ev=i32(ev), nu=i32(np.full(S, n)), ptr=i32(in_ptr), edge=i32(in_edge), level=i32(self.level), level_node=i32(level_node),
                      colour_node=i32(colour_node), g=torch.as_tensor(g).to(dev), score=torch.zeros((S, n), **f64), d2=d2, K=torch.empty_like(d2),
                      w=torch.empty((S, n), **f64), mu=torch.empty((2, 2 * E, n), **f64), resid=torch.empty((most, 2 * E), **f64),
                      belief=torch.empty((S, n), **f64), state=torch.empty(S, dtype=torch.int32, device=dev), res=torch.empty(most, **f64),
                      mm=torch.empty((S, n), **f64), decoded=torch.zeros(S, dtype=torch.int32, device=dev),
                      moves=torch.zeros((1, most), dtype=torch.int32, device=dev))
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def sum_product(self, sweeps):
        p = {name: v.data_ptr() for name, v in self.t.items()}
        _lib.check(self.lib.gbp_section_propagate(self.S, self.E, self.n, p["eu"], p["ev"], p["nu"], p["score"], p["g"], p["d2"], p["ptr"], p["edge"], sweeps, 0.0,
                                                  p["K"], p["w"], p["mu"], p["resid"], p["belief"], p["state"], p["res"], self.stream))

    def max_sum(self, sweeps):
        p = {name: v.data_ptr() for name, v in self.t.items()}
        _lib.check(self.lib.gbp_section_graph_path(self.S, self.E, self.n, p["eu"], p["ev"], p["nu"], p["score"], p["g"], p["d2"], p["ptr"], p["edge"], sweeps, 0.0,
                                                   self.level_ptr.size - 1, np.ctypeslib.as_ctypes(self.level_ptr), p["level_node"], p["level"], p["mu"],
                                                   p["resid"], p["mm"], p["decoded"], p["res"], self.stream))

    def refine(self, sweeps):
        p = {name: v.data_ptr() for name, v in self.t.items()}
        _lib.check(self.lib.gbp_section_graph_refine(self.S, self.E, self.n, 1, p["eu"], p["ev"], p["nu"], p["score"], p["g"], p["d2"], p["ptr"], p["edge"],
                                                     self.colour_ptr.size - 1, np.ctypeslib.as_ctypes(self.colour_ptr), p["colour_node"], sweeps, p["decoded"],
                                                     p["moves"], self.stream))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--lines", type=int, default=40)
    p.add_argument("--soundings", type=int, default=250, help="per line")
    p.add_argument("--models", type=int, default=64)
    p.add_argument("--line", type=int, default=4000, help="the soundings of the one long line the decode is timed on")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sweeps", type=int, default=32, help="the sweeps the per-sweep time is taken over")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "spatial_path", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spatial_path needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    n = a.models
    k, edges, sigma, x, y, ptr = synthetic_survey(a.lines, a.soundings, n, a.seed)
    S = k.shape[0]
    ens = Ensemble(torch.as_tensor(k).to(dev), torch.as_tensor(edges).to(dev), torch.as_tensor(sigma).to(dev), None, None, 1, None)
    rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(S, n).contiguous()
    eu, ev, g, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * ACROSS)
    E = int(eu.size)
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count,
                  lines=a.lines, soundings_per_line=a.soundings, soundings=S, models=n, edges=E, rounds=a.rounds, warmup=a.warmup, sweeps_timed=a.sweeps)
    d2 = sections.edge_distance(ens, rows, eu, ev, 0.0, Z1)
    # what the path is worth on this survey: the belief argmax against the path, one call each
    belief = sections.propagate(d2, g, eu, ev, np.full(S, n), S, sweeps=a.sweeps)
    found = sections.graph_path(d2, g, eu, ev, np.full(S, n), S, sweeps=a.sweeps, candidates=belief["state"][None, :])
    residual = found["residual"].cpu().numpy()
    result.update(log_score=dict(belief_argmax=float(sections.graph_log_score(belief["state"][None, :], None, torch.as_tensor(g).to(dev), d2,
                                                                              torch.as_tensor(eu).to(dev), torch.as_tensor(ev).to(dev))[0]),
                                 candidates_refined=[float(v) for v in found["candidate_log_score"].cpu().numpy()], chosen=int(found["chosen"])),
                  soundings_changed=int((found["state"] != belief["state"]).sum()), refine_moves=found["refine_moves"].cpu().numpy().tolist(),
                  max_sum_residual={str(t): float(residual[t - 1]) for t in (1, 2, 5, 10, 20, 32) if t <= residual.size})
    del belief, found
    survey = Graph(eu, ev, g, d2, S, n, 1 + a.sweeps, dev)
    slab = E * n * n * 8
    one_sp, many_sp, sweep_sp = timed(survey.sum_product, a.sweeps, a.rounds, a.warmup, dev)
    one_ms, many_ms, sweep_ms = timed(survey.max_sum, a.sweeps, a.rounds, a.warmup, dev)
    survey.t["decoded"].zero_()
    _, _, sweep_refine = timed(survey.refine, a.sweeps, a.rounds, a.warmup, dev)
    result.update(bytes_per_sweep=slab, floor_seconds_per_sweep=dict(hbm_peak=slab / HBM_PEAK, hbm_achievable=slab / HBM_ACHIEVABLE),
                  sum_product=dict(ms_one_sweep_call=one_sp, ms_many_sweep_call=many_sp, seconds_per_sweep=sweep_sp),
                  max_sum=dict(ms_one_sweep_call=one_ms, ms_many_sweep_call=many_ms, seconds_per_sweep=sweep_ms,
                               seconds_once=one_ms * 1e-3 - sweep_ms, levels=int(survey.level_ptr.size - 1)),
                  max_sum_over_sum_product=sweep_ms / sweep_sp if sweep_sp > 0 else None,
                  refine=dict(seconds_per_sweep=sweep_refine, colours=int(survey.colour_ptr.size - 1)))
    del survey, d2
    # the decode where it is longest: one line, a level per sounding
    N = a.line
    rng = np.random.default_rng(a.seed + 1)
    leu, lev = np.arange(N - 1), np.arange(1, N)
    line = Graph(leu, lev, rng.uniform(5.0, 60.0, N - 1), torch.as_tensor(rng.uniform(0.0, 0.3, (N - 1, n, n))).to(dev), N, n, 1 + a.sweeps, dev)
    one_l, many_l, sweep_l = timed(line.max_sum, a.sweeps, a.rounds, a.warmup, dev)
    levels = int(line.level_ptr.size - 1)
    result.update(long_line=dict(soundings=N, levels=levels, ms_one_sweep_call=one_l, seconds_per_sweep=sweep_l, seconds_decode=one_l * 1e-3 - sweep_l,
                                 seconds_per_level=(one_l * 1e-3 - sweep_l) / levels,
                                 note="seconds_decode is the one-sweep call less one sweep: the decode's launches with the three that run once"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({name: result[name] for name in ("edges", "sum_product", "max_sum", "max_sum_over_sum_product", "refine", "long_line", "log_score")}))
    return result


if __name__ == "__main__":
    main()
