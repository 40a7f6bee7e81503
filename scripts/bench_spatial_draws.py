"""Joint draws across flight lines (gbp_section_graph_draw): what a sweep of line-blocked Gibbs sampling costs on
the survey of bench_spatial_sections.py (40 lines x 250 soundings, n = 64, max_distance = 1.5 line spacings), and how the chains move.

The C entry is timed on preallocated buffers between device events, medians after warm-up rounds, K ready: the start sweep alone
(first_sweep = last_sweep = 0) and the start with SWEEPS conditioned sweeps taking turns in one process; seconds per conditioned sweep
is the difference over SWEEPS.  The split between the filter and the draw launches is read from one profiled call (torch.profiler's
device activities; null where the profiler is not available).  Beside them stand two floors per sweep: arithmetic, R S n^2 fused
multiply-adds at the fp64 vector rate, and traffic, the K of the steps read once (every line lies in one colour class) at the
streaming-copy rate of bench_spatial_sections.py.  One traced run of 64 sweeps gives ``change_share`` and the mean log score per
sweep, and the draws after the default 8 sweeps give the largest |draw_share - weight| against the beliefs of 32 sweeps of message
passing.  There is no pass / fail threshold: nothing here has a parent number; the numbers go into DESIGN.md 3.29.  Writes one JSON file.

    python scripts/bench_spatial_draws.py [--lines 40] [--soundings 250] [--models 64] [--draws 64] [--sweeps 8] [--trace-sweeps 64]
                                          [--rounds 5] [--warmup 2] [--seed 0] [--out profiles/spatial_draws/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_spatial_sections import ACROSS, HBM_ACHIEVABLE, Z1, events_ms, synthetic_survey      # noqa: E402
from geobipy_amd import _lib, sections      # noqa: E402
from geobipy_amd.ensembles import Ensemble      # noqa: E402

FP64_FMA_PER_SECOND = 78.6e12 / 2.0                                            # the fp64 vector peak, counted in fused multiply-adds


def kernel_split(call, dev):
    """{kernel name: device microseconds} of one call, through torch.profiler; None if it records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize(dev)
        out = {}
        for ev in prof.key_averages():
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            if "k_graph_line" in ev.key and us > 0.0:
                out["filter" if "filter" in ev.key else "draw"] = out.get("filter" if "filter" in ev.key else "draw", 0.0) + us
        return out or None
    except Exception as e:      # noqa: BLE001  (a measurement aid: its absence is recorded, not fatal)
        return dict(error=repr(e))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--lines", type=int, default=40)
    p.add_argument("--soundings", type=int, default=250, help="per line")
    p.add_argument("--models", type=int, default=64)
    p.add_argument("--draws", type=int, default=64)
    p.add_argument("--sweeps", type=int, default=8, help="the conditioned sweeps the per-sweep time is taken over")
    p.add_argument("--trace-sweeps", type=int, default=64)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "spatial_draws", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spatial_draws needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    n, R, T = a.models, a.draws, a.sweeps
    k, edges, sigma, x, y, ptr = synthetic_survey(a.lines, a.soundings, n, a.seed)
    S, L = k.shape[0], a.lines
    ens = Ensemble(torch.as_tensor(k).to(dev), torch.as_tensor(edges).to(dev), torch.as_tensor(sigma).to(dev), None, None, 1, None)
    rows = torch.arange(n, dtype=torch.int32, device=dev)[None, :].expand(S, n).contiguous()
    eu, ev, g, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * ACROSS)
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    E, nu = int(eu.size), np.full(S, n)
    d2 = sections.edge_distance(ens, rows, eu, ev, 0.0, Z1)
    beliefs = sections.propagate(d2, g, eu, ev, nu, S, sweeps=32, keep_kernel=True)
    K = beliefs["kernel"]
    _, step_edge, cross = sections.check_lines(eu, ev, ptr, S, "bench_spatial_draws")
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count, lines=L,
                  soundings_per_line=a.soundings, soundings=S, models=n, edges=E, cross_edges=int(cross.sum()), n_colours=n_colours, draws=R,
                  sweeps_timed=T, rounds=a.rounds, warmup=a.warmup)
    cross_ptr, cross_edge = sections.cross_incoming(eu, ev, cross, S)
    i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(dev)      # noqa: E731
    t_eu, t_ev, t_nu, t_step, t_cptr, t_cedge = i32(eu), i32(ev), i32(nu), i32(step_edge), i32(cross_ptr), i32(np.concatenate([cross_edge, [-1]]))
    t_colptr, t_colline = i32(np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))])), i32(np.argsort(colour, kind="stable"))
    t_ptr = torch.as_tensor(ptr.astype(np.int64)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    score, w, alpha, scale = torch.zeros((S, n), **f64), torch.empty((S, n), **f64), torch.empty((R, S, n), **f64), torch.empty((R, S), **f64)
    state = torch.zeros((R, S), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(first, last):
        _lib.check(lib.gbp_section_graph_draw(S, E, n, L, t_ptr.data_ptr(), t_eu.data_ptr(), t_ev.data_ptr(), t_nu.data_ptr(), score.data_ptr(), None, None, 1,
                                              K.data_ptr(), t_step.data_ptr(), t_cptr.data_ptr(), t_cedge.data_ptr(), n_colours, t_colptr.data_ptr(),
                                              t_colline.data_ptr(), None, a.seed, R, 0, first, last, w.data_ptr(), alpha.data_ptr(), scale.data_ptr(),
                                              state.data_ptr(), stream))

    t = {0: [], T: []}
    for r in range(a.warmup + a.rounds):
        for last in (0, T):                                                   # taking turns
            ms = events_ms(lambda: call(0, last), dev)
            if r >= a.warmup:
                t[last].append(ms)
    start, whole = float(np.median(t[0])), float(np.median(t[T]))
    per_sweep = (whole - start) / T * 1e-3
    step_bytes = int((step_edge >= 0).sum()) * n * n * 8
    result.update(ms_start_call=t[0], ms_start_and_sweeps_call=t[T], seconds_start_sweep=start * 1e-3, seconds_per_conditioned_sweep=per_sweep,
                  microseconds_by_launch=dict(start_sweep=kernel_split(lambda: call(0, 0), dev), one_conditioned_sweep=kernel_split(lambda: call(1, 1), dev)),
                  floor_seconds_per_sweep=dict(arithmetic_fp64_vector=R * S * n * n / FP64_FMA_PER_SECOND, traffic_step_K_once=step_bytes / HBM_ACHIEVABLE),
                  bytes_K=E * n * n * 8, bytes_step_K=step_bytes)
    traced = sections.graph_draw(d2, g, eu, ev, nu, ptr, R, seed=a.seed, sweeps=a.trace_sweeps, kernel=K, trace=True, filtered=False)
    result.update(change_share=traced["change_share"].cpu().numpy().tolist(), mean_log_score=traced["log_score_trace"].mean(dim=1).cpu().numpy().tolist())
    drawn = sections.graph_draw(d2, g, eu, ev, nu, ptr, R, seed=a.seed, sweeps=8, kernel=K, filtered=False)["draw_state"].long()
    share = torch.zeros((S, n), **f64).scatter_add_(1, drawn.t().contiguous(), torch.ones((S, R), **f64)) / R
    gap = (share - beliefs["belief"]).abs()
    result.update(largest_draw_share_minus_weight=float(gap.max()), mean_draw_share_minus_weight=float(gap.mean()),
                  binomial_sd_at_half=float(0.5 / np.sqrt(R)), same_state_as_beliefs=float((drawn == beliefs["state"].long()[None, :]).double().mean()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({name: result[name] for name in ("seconds_start_sweep", "seconds_per_conditioned_sweep", "microseconds_by_launch", "floor_seconds_per_sweep",
                                                      "largest_draw_share_minus_weight")}))
    return result


if __name__ == "__main__":
    main()
