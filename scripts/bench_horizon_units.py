"""Time of the horizon-pair tracker (csrc/gbp_horizon_unit.h k_unit_viterbi, k_unit_marginals) on a survey-sized launch -- 8 lines of
1 000 soundings and S = horizons.MAX_UNIT_STATES cells, a planted dipping unit under terrain with 30 % of the evidence of each horizon
at a wrong depth:

    python scripts/bench_horizon_units.py [--sequences 8 --soundings 1000 --states 96] [--reps 5] [--check 16]
                                          [--out profiles/horizon_units/bench.json]

gbp_horizon_unit_track without marginals (the Viterbi kernel and its walk back), with marginals (both kernels), and with the absent
state and marginals, through the C entry on preallocated inputs and workspaces, timed with device events, the candidates alternating
inside each repetition of one process; medians after a warm-up.  The picks and the marginals are held to the numpy rule on the first
``--check`` soundings of the first line (a chain cut short is a chain of its own).  There is no yardstick to beat: the S^2-state chain
has no other formulation in the package, and the two tracks alone (scripts/bench_horizons.py) answer another question.  No counters
are taken.  Prints one line per measurement and writes them as JSON to --out."""
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
from geobipy_amd import _lib, horizons  # noqa: E402


def planted(L, N, S, dz, seed):
    """Evidence of the top and of the base [L N, S], x, surface [L N] of L lines with a dipping unit 5 .. 15 cells thick; 30 % of the
    soundings of each horizon point at a random cell."""
    rng = np.random.default_rng(seed)
    x = np.tile(25.0 * np.arange(N), L)
    phase = np.repeat(rng.uniform(0.0, 6.0, L), N)
    surface = 5.0 * np.sin(x / 1500.0 + phase) + rng.normal(0.0, 0.3, L * N)
    depth = surface + 0.35 * S * dz - 3.0 * np.sin(x / 2000.0 + phase)
    top = np.clip(np.floor(depth / dz), 0, S - 16).astype(np.int64)
    base = top + 10 + np.round(5.0 * np.sin(x / 900.0 + phase)).astype(np.int64)
    out = []
    for true in (top, base):
        at = np.where(rng.uniform(size=L * N) < 0.3, rng.integers(0, S, L * N), true)
        out.append(0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2))
    return out[0], out[1], x, surface, top, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=8)
    ap.add_argument("--soundings", type=int, default=1000)
    ap.add_argument("--states", type=int, default=horizons.MAX_UNIT_STATES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=16, help="soundings of the first line held to the numpy rule")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L, N, S, dz, slope, switch, mc = a.sequences, a.soundings, a.states, 0.5, 0.05, 4.6, 1
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e_top, e_base, x, surface, top, base = planted(L, N, S, dz, 7)
    ptr = np.arange(L + 1, dtype=np.int64) * N
    st_h, sb_h = horizons.evidence_scores(e_top)[0], horizons.evidence_scores(e_base)[0]
    absent_h = np.full(L * N, 2.0 * np.log(0.01))
    g_h, d_h = horizons.steps(x, np.zeros(L * N), surface, slope, ptr=ptr)
    t = lambda v, dt=torch.float64: torch.as_tensor(v, dtype=dt).to(dev)                   # noqa: E731
    st, sb, absent, g, d, tptr = t(st_h), t(sb_h), t(absent_h), t(g_h), t(d_h), t(ptr, torch.int64)
    f64 = dict(dtype=torch.float64, device=dev)
    back = torch.empty((2, L * N, S, S), dtype=torch.uint8, device=dev)
    back_absent = torch.empty(L * N, dtype=torch.int32, device=dev)
    cell_top, cell_base = torch.empty(L * N, dtype=torch.int32, device=dev), torch.empty(L * N, dtype=torch.int32, device=dev)
    log_score = torch.empty(L, **f64)
    alpha = torch.empty((L * N, S * S + 1), **f64)
    m_top, m_base, m_thick = (torch.empty((L * N, S), **f64) for _ in range(3))
    m_absent, log_partition, scale = torch.empty(L * N, **f64), torch.empty(L, **f64), torch.empty(L * N, **f64)

    def kernel(with_marginals, with_absent=False):
        p = (lambda v: v.data_ptr()) if with_marginals else (lambda v: None)
        _lib.check(lib.gbp_horizon_unit_track(L, tptr.data_ptr(), L * N, N, S, mc, dz, st.data_ptr(), sb.data_ptr(), None,
                                              absent.data_ptr() if with_absent else None, g.data_ptr(), d.data_ptr(), switch, back.data_ptr(),
                                              back_absent.data_ptr(), cell_top.data_ptr(), cell_base.data_ptr(), log_score.data_ptr(), p(alpha),
                                              p(m_top), p(m_base), p(m_thick), p(m_absent), p(log_partition), p(scale), stream))

    r = dict(sequences=L, soundings=N, states=S, min_cells=mc, reps=a.reps, device=torch.cuda.get_device_name(0),
             workspace_bytes=horizons.unit_bytes(L * N, S, True))
    times = alternating({"kernel_viterbi": lambda: kernel(False), "kernel_both": lambda: kernel(True),
                         "kernel_both_absent": lambda: kernel(True, True)}, a.reps, warmup=1)
    for k, ms in times.items():
        r[k + "_ms"] = ms
    r["kernel_marginals_ms"] = times["kernel_both"] - times["kernel_viterbi"]
    r["kernel_viterbi_us_per_step"] = times["kernel_viterbi"] * 1e3 / (N - 1)
    r["kernel_marginals_us_per_step"] = r["kernel_marginals_ms"] * 1e3 / (N - 1)
    r["max_adds_per_launch"] = float(L) * (N - 1) * 2.0 * S * S * S
    kernel(True)
    torch.cuda.synchronize()
    ct, cb = cell_top.view(L, N).cpu().numpy(), cell_base.view(L, N).cpu().numpy()
    r["ordered_everywhere"] = bool(np.all(cb - ct >= mc))
    r["top_mean_error_cells"] = float(np.abs(ct - top.reshape(L, N)).mean())
    r["base_mean_error_cells"] = float(np.abs(cb - base.reshape(L, N)).mean())
    r["argmax_pairs_crossed_share"] = float(np.mean(np.argmax(e_base, axis=1) - np.argmax(e_top, axis=1) < mc))
    # the first soundings of the first line as a chain of their own, against the rule
    n = min(a.check, N)
    if n:
        got = horizons._unit_launch(st[:n], sb[:n], None, None, np.array([0, n]), g_h[:n], d_h[:n], dz, switch, mc, True)
        ref = horizons.unit_reference([0, n], st_h[:n], sb_h[:n], g_h[:n], d_h[:n], dz, switch, min_cells=mc)
        ld = horizons.unit_reference([0, n], st_h[:n], sb_h[:n], g_h[:n], d_h[:n], dz, switch, min_cells=mc, dtype=np.longdouble)
        keys = ("marginal_top", "marginal_base", "marginal_thickness")
        e = max(float(np.abs(ref[k] - ld[k]).max()) for k in keys)
        dist = max(float(np.abs(got[k].cpu().numpy() - ld[k]).max()) for k in keys)
        r.update(checked_soundings=n, rule_own_rounding_e=e, marginal_max_distance_to_long_double_rule=dist,
                 picks_equal_the_rule=bool(np.array_equal(got["cell_top"].cpu().numpy(), ref["cell_top"])
                                           and np.array_equal(got["cell_base"].cpu().numpy(), ref["cell_base"])
                                           and np.array_equal(got["log_score"].cpu().numpy(), ref["log_score"])))
    r["not_measured"] = "hardware counters, other launch sizes, more than one device"
    for k, v in r.items():
        print("%s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
