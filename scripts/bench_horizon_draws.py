"""Time of the joint draws of horizons along lines (csrc/gbp_horizon_draw.h k_horizon_filter, k_horizon_walk) beside the line tracker
with marginals (csrc/gbp_horizon.h) at the same state counts:

    python scripts/bench_horizon_draws.py [--states 64 440 2048] [--draws 256] [--reps 7] [--out profiles/horizon_draws/bench.json]

64 sequences of 129 soundings with the absent state, as scripts/bench_horizon_graph.py runs the tracker: gbp_horizon_draw with
``--draws`` realisations and with one, gbp_horizon_track with and without marginals.  Every candidate runs on preallocated buffers and
is timed with device events, the candidates alternating inside each repetition of one process; medians of ``--reps`` after 2 warm-up
rounds.  The entry launches the filter and the walk back to back, so the two kernels are told apart by the profiler's kernel records
(torch.profiler; medians over the same number of calls), where it is available: ``filter_ms`` and ``walk_ms`` are null where it is not.
One conditioned sweep of the graph draws (gbp_horizon_graph_draw) on the benchmark survey of scripts/bench_horizon_graph.py -- 8 lines of
128 soundings 25 m apart, 100 m between lines, joined across up to 150 m -- with ``--graph-draws`` = 64 realisations: calls that
continue with 1 and with 5 sweeps, the difference over 4 being a sweep (all colours: a conditioned filter and a walk each).
There is no speed bar: no kernel here has a parent, and the tracker's times are printed beside for reading.  Prints one JSON line per
state count and writes them to --out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_horizon_graph import DZ, SLOPE, SWITCH, track  # noqa: E402
from bench_intervals import alternating  # noqa: E402
from geobipy_amd import _lib, horizons, sections  # noqa: E402


def draw(L, N, S, R, dev):
    """gbp_horizon_draw with the absent state on L sequences of N soundings: the inputs of ``bench_horizon_graph.track``."""
    rng = np.random.default_rng(7)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    x = np.tile(25.0 * np.arange(N), L)
    surface = 10.0 * np.sin(x / 1500.0) + rng.normal(0.0, 0.3, L * N)
    ptr = np.arange(L + 1, dtype=np.int64) * N
    g, d = horizons.steps(x, np.zeros(L * N), surface, SLOPE, ptr=ptr)
    t = lambda v, dt=torch.float64: torch.as_tensor(v, dtype=dt).to(dev)                  # noqa: E731
    score, absent, g, d, tptr = t(rng.normal(size=(L * N, S))), t(np.full(L * N, np.log(0.01))), t(g), t(d), t(ptr, torch.int64)
    filtered, scale = torch.empty((L * N, S + 1), dtype=torch.float64, device=dev), torch.empty(L * N, dtype=torch.float64, device=dev)
    state = torch.empty((R, L * N), dtype=torch.int32, device=dev)

    def run(n_draws):
        _lib.check(lib.gbp_horizon_draw(L, tptr.data_ptr(), L * N, N, S, DZ, score.data_ptr(), absent.data_ptr(), g.data_ptr(), d.data_ptr(), SWITCH,
                                        None, 11, n_draws, filtered.data_ptr(), scale.data_ptr(), state.data_ptr(), stream))
    return run


def graph_draw(lines, n, S, R, dev, seed=3):
    """gbp_horizon_graph_draw on the survey of ``bench_horizon_graph.Graph``: run(first_sweep, sweeps) continues from the start's states."""
    rng = np.random.default_rng(seed)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    x, y, ptr = np.tile(25.0 * np.arange(n), lines), np.repeat(100.0 * np.arange(lines), n), np.arange(lines + 1, dtype=np.int64) * n
    N = x.size
    surface = 10.0 * np.sin(x / 1500.0) + 0.01 * y + rng.normal(0.0, 0.3, N)
    eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=150.0)
    g, d, _ = horizons.graph_steps(x, y, surface, eu, ev, SLOPE)
    at = np.clip(np.floor((surface + 0.25 * S * DZ) / DZ), 0, S - 1)
    score = np.concatenate([horizons.evidence_scores(0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2))[0],
                            np.full((N, 1), np.log(0.01))], axis=1)
    _, step_edge, cross = sections.check_lines(eu, ev, ptr, N, "bench")
    cross_ptr, cross_edge = sections.cross_incoming(eu, ev, cross, N)
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    colour_ptr = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))])
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(dev)          # noqa: E731
    i = [t(v, torch.int32) for v in (eu, ev, step_edge, cross_ptr, cross_edge, colour_ptr, np.argsort(colour, kind="stable"))]
    f = [t(v, torch.float64) for v in (score, g, d)]
    tptr = t(ptr, torch.int64)
    alpha, scale = torch.empty((R, N, S + 1), dtype=torch.float64, device=dev), torch.empty((R, N), dtype=torch.float64, device=dev)
    state = torch.zeros((R, N), dtype=torch.int32, device=dev)
    p = lambda v: v.data_ptr()                                                            # noqa: E731

    def run(first_sweep, sweeps):
        _lib.check(lib.gbp_horizon_graph_draw(N, eu.size, S, 1, DZ, SWITCH, p(i[0]), p(i[1]), p(f[0]), p(f[1]), p(f[2]), lines, p(tptr), p(i[2]), p(i[3]),
                                              p(i[4]), n_colours, p(i[5]), p(i[6]), None, 11, R, 0, first_sweep, sweeps, p(alpha), p(scale), p(state),
                                              stream))
    run(0, 0)                                                                             # the start: states to continue from
    return run, dict(graph_soundings=N, graph_edges=int(eu.size), graph_cross_edges=int(cross.sum()), graph_colours=n_colours,
                     graph_alpha_bytes=R * N * (S + 1) * 8)


def kernels_apart(fn, reps):
    """{kernel name fragment: median ms} of the filter and the walk over ``reps`` calls of ``fn``, from the profiler's kernel records;
    None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        found = {"k_horizon_filter": [], "k_horizon_walk": []}
        for _ in range(reps):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            for name in found:
                us = [e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in prof.events() if name in e.name]
                if us:
                    found[name].append(sum(us) * 1e-3)
        return {k: (statistics.median(v) if v else None) for k, v in found.items()}
    except Exception as e:                                                               # noqa: BLE001  (no profiler: the split stays unknown)
        print("kernels_apart: %s" % e, file=sys.stderr)
        return {"k_horizon_filter": None, "k_horizon_walk": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, nargs="+", default=[64, 440, 2048])
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--graph-draws", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L, N, R = 64, 129, a.draws
    rows = []
    for S in a.states:
        line, drawn = track(L, N, S, dev), draw(L, N, S, R, dev)
        graph, shape = graph_draw(8, 128, S, a.graph_draws, dev)
        times = alternating({"draw": lambda: drawn(R), "draw_one": lambda: drawn(1), "track_viterbi": lambda: line(False),
                             "track_both": lambda: line(True), "graph_sweeps_1": lambda: graph(1, 1), "graph_sweeps_5": lambda: graph(1, 5)},
                            a.reps, warmup=2)
        apart = kernels_apart(lambda: drawn(R), a.reps)
        r = dict(states=S, sequences=L, soundings=N, draws=R, reps=a.reps, device=torch.cuda.get_device_name(0),
                 draw_us_per_step=times["draw"] * 1e3 / (N - 1), draw_one_us_per_step=times["draw_one"] * 1e3 / (N - 1),
                 track_marginals_alone_us_per_step=(times["track_both"] - times["track_viterbi"]) * 1e3 / (N - 1),
                 filter_ms=apart["k_horizon_filter"], walk_ms=apart["k_horizon_walk"], graph_draws=a.graph_draws,
                 graph_conditioned_sweep_ms=(times["graph_sweeps_5"] - times["graph_sweeps_1"]) / 4.0, **shape)
        r.update({k + "_ms": v for k, v in times.items()})
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
