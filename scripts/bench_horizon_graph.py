"""Time of a sweep of the horizon graph (csrc/gbp_horizon_graph.h k_hgraph_sweep, both semirings) beside the step of the line tracker
(csrc/gbp_horizon.h) at the same state counts:

    python scripts/bench_horizon_graph.py [--lines 8 --soundings 128] [--states 64 440 2048] [--reps 7] [--out profiles/horizon_graph/bench.json]

  (a) a survey of ``--lines`` lines 100 m apart with ``--soundings`` soundings 25 m apart, joined across up to 150 m
      (``sections.neighbours``): gbp_horizon_graph_propagate and gbp_horizon_graph_path through the C entries with 1 and with 33 sweeps;
      the difference over 32 is a sweep, and over the edges a sweep per edge at full occupancy of the device;
  (b) the same on a graph of 64 edges (a path of 65 soundings): fewer workgroups than CUs, so a sweep is the latency of ONE edge, the
      number to put beside
  (c) gbp_horizon_track with marginals on 64 sequences of 129 soundings, per step: 64 workgroups, each alone on its CU, walk one
      forward and one backward O(S^2) pass per step where a sweep walks two O(S^2) passes per edge.

Every candidate runs on preallocated buffers and is timed with device events, the candidates alternating inside each repetition of one
process; medians after a warm-up.  Prints one JSON line per state count and writes them to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_intervals import alternating  # noqa: E402
from geobipy_amd import _lib, horizons, sections  # noqa: E402

DZ, SLOPE, SWITCH, SWEEPS = 0.5, 0.05, 4.6, 33


class Graph:
    """The device buffers of one graph at one state count and the two entries on them."""

    def __init__(self, x, y, ptr, S, dev, seed=3):
        rng = np.random.default_rng(seed)
        self.lib, self.stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
        N = x.size
        surface = 10.0 * np.sin(x / 1500.0) + 0.01 * y + rng.normal(0.0, 0.3, N)
        eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=150.0)
        g, d, _ = horizons.graph_steps(x, y, surface, eu, ev, SLOPE)
        at = np.clip(np.floor((surface + 0.25 * S * DZ) / DZ), 0, S - 1)
        score = np.concatenate([horizons.evidence_scores(0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2))[0],
                                np.full((N, 1), np.log(0.01))], axis=1)
        in_ptr, in_edge = sections.incoming(eu, ev, N)
        level, self.level_ptr, level_node = sections.decode_levels(eu, ev, N)
        t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(dev)      # noqa: E731
        self.N, self.E, self.S, SA = N, eu.size, S, S + 1
        self.i = [t(v, torch.int32) for v in (eu, ev, in_ptr, in_edge, level_node, level)]
        self.f = [t(v, torch.float64) for v in (score, g, d)]
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
        self.w, self.msg, self.resid, self.out, self.residual = f64(N, SA), f64(2, 2 * self.E, SA), f64(SWEEPS, 2 * self.E), f64(N, SA), f64(SWEEPS)
        self.state = torch.empty(N, dtype=torch.int32, device=dev)

    def propagate(self, sweeps):
        (eu, ev, in_ptr, in_edge, _, _), (score, g, d), p = self.i, self.f, lambda v: v.data_ptr()
        _lib.check(self.lib.gbp_horizon_graph_propagate(self.N, self.E, self.S, 1, DZ, SWITCH, p(eu), p(ev), p(score), p(g), p(d), p(in_ptr), p(in_edge), sweeps,
                                                        0.0, p(self.w), p(self.msg), p(self.resid), p(self.out), p(self.state), p(self.residual), self.stream))

    def path(self, sweeps):
        (eu, ev, in_ptr, in_edge, level_node, level), (score, g, d), p = self.i, self.f, lambda v: v.data_ptr()
        _lib.check(self.lib.gbp_horizon_graph_path(self.N, self.E, self.S, 1, DZ, SWITCH, p(eu), p(ev), p(score), p(g), p(d), p(in_ptr), p(in_edge), sweeps, 0.0,
                                                   self.level_ptr.size - 1, np.ctypeslib.as_ctypes(self.level_ptr), p(level_node), p(level), p(self.msg),
                                                   p(self.resid), p(self.out), p(self.state), p(self.residual), self.stream))


def track(L, N, S, dev):
    """gbp_horizon_track with marginals and the absent state on L sequences of N soundings, as scripts/bench_horizons.py runs it."""
    rng = np.random.default_rng(7)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    x = np.tile(25.0 * np.arange(N), L)
    surface = 10.0 * np.sin(x / 1500.0) + rng.normal(0.0, 0.3, L * N)
    ptr = np.arange(L + 1, dtype=np.int64) * N
    g, d = horizons.steps(x, np.zeros(L * N), surface, SLOPE, ptr=ptr)
    t = lambda v, dt=torch.float64: torch.as_tensor(v, dtype=dt).to(dev)                  # noqa: E731
    score, absent, g, d, tptr = t(rng.normal(size=(L * N, S))), t(np.full(L * N, np.log(0.01))), t(g), t(d), t(ptr, torch.int64)
    back = torch.empty((L * N, S + 1), dtype=torch.int16, device=dev)
    cell, log_score = torch.empty(L * N, dtype=torch.int32, device=dev), torch.empty(L, dtype=torch.float64, device=dev)
    marginal, log_partition, scale = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((L * N, S + 1), (L,), (L * N,)))

    def run(with_marginals):
        p = (lambda v: v.data_ptr()) if with_marginals else (lambda v: None)
        _lib.check(lib.gbp_horizon_track(L, tptr.data_ptr(), L * N, N, S, DZ, score.data_ptr(), absent.data_ptr(), g.data_ptr(), d.data_ptr(), SWITCH,
                                         back.data_ptr(), cell.data_ptr(), log_score.data_ptr(), p(marginal), p(log_partition), p(scale), stream))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=8)
    ap.add_argument("--soundings", type=int, default=128)
    ap.add_argument("--states", type=int, nargs="+", default=[64, 440, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L, n, TL, TN = a.lines, a.soundings, 64, 129
    sx, sy = np.tile(25.0 * np.arange(n), L), np.repeat(100.0 * np.arange(L), n)
    rows = []
    for S in a.states:
        survey = Graph(sx, sy, np.arange(L + 1) * n, S, dev)
        one = Graph(25.0 * np.arange(65), np.zeros(65), None, S, dev)
        line = track(TL, TN, S, dev)
        times = alternating({"survey_sum_1": lambda: survey.propagate(1), "survey_sum_n": lambda: survey.propagate(SWEEPS),
                             "survey_max_1": lambda: survey.path(1), "survey_max_n": lambda: survey.path(SWEEPS),
                             "path64_sum_1": lambda: one.propagate(1), "path64_sum_n": lambda: one.propagate(SWEEPS),
                             "path64_max_1": lambda: one.path(1), "path64_max_n": lambda: one.path(SWEEPS),
                             "track_viterbi": lambda: line(False), "track_both": lambda: line(True)}, a.reps, warmup=2)
        r = dict(states=S, survey_soundings=survey.N, survey_edges=survey.E, reps=a.reps, device=torch.cuda.get_device_name(0),
                 message_bytes=horizons.message_bytes(survey.E, S + 1))
        for kind in ("sum", "max"):
            sweep = (times["survey_%s_n" % kind] - times["survey_%s_1" % kind]) / (SWEEPS - 1)
            r["survey_%s_sweep_ms" % kind] = sweep
            r["survey_%s_us_per_edge" % kind] = sweep * 1e3 / survey.E
            r["edge_%s_latency_us" % kind] = (times["path64_%s_n" % kind] - times["path64_%s_1" % kind]) * 1e3 / (SWEEPS - 1)
        r["track_with_marginals_us_per_step"] = times["track_both"] * 1e3 / (TN - 1)
        r["track_marginals_alone_us_per_step"] = (times["track_both"] - times["track_viterbi"]) * 1e3 / (TN - 1)
        r.update({k + "_ms": v for k, v in times.items()})
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
