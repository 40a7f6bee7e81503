"""Horizons across flight lines, the rules alone (geobipy_amd.horizons graph_steps, propagate_reference, graph_path_reference,
refine_reference, graph_log_score): no GPU.

The rules are held to what they must equal where that is known: ``track_reference`` on a line graph (the smoothed marginals within
16 max(e, U) of the long-double ones, e the fp64 rule's own distance from the rule in long double and U = 2^-53; the decode ``==`` the
Viterbi path) and brute-force enumeration on a star and on a small lattice.  Every case prints used / bound."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, horizons, sections
from test_spatial_sections import lattice_graph, star_graph

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- what both test files use ----------------------------------------------------------------------------------------------------------

def horizon_inputs(rng, eu, ev, N, S, absent, dz=0.5, slope=0.5):
    """score [N, S], absent_score [N] or None, g, d [E] through ``graph_steps`` from soundings 3 .. 12 m apart on a rough surface.  With
    two edges or more the first edge has a zero distance (clamped to min_distance: g = 1 / slope) and the last has |d| > S dz."""
    x, y = np.cumsum(rng.uniform(3.0, 12.0, N)), rng.uniform(-5.0, 5.0, N)
    surface = rng.normal(size=N) * min(S, 8) * dz * 0.3
    E = len(eu)
    if E >= 2:
        x[ev[0]], y[ev[0]] = x[eu[0]], y[eu[0]]
        surface[ev[-1]] = surface[eu[-1]] + (S + 0.7) * dz * (1.0 if ev[-1] % 2 else -1.0)
    g, d, dist = horizons.graph_steps(x, y, surface, eu, ev, slope=slope)
    if E >= 2:
        assert dist[0] == 0.0 and g[0] == 1.0 / slope and abs(d[-1]) > S * dz
    return rng.normal(size=(N, S)), (rng.normal(size=N) if absent else None), g, d, dz


def brute_force(eu, ev, g, d, dz, switch, score, absent_score):
    """(marginals [N, SA], the first mode in lexicographic order, its log score, all log scores) by enumeration, in long double."""
    ft = np.longdouble
    N, S = score.shape
    theta = score if absent_score is None else np.concatenate([score, absent_score[:, None]], axis=1)
    SA = theta.shape[1]
    marg, best, best_cfg, every = np.zeros((N, SA), dtype=ft), -np.inf, None, []
    for cfg in itertools.product(range(SA), repeat=N):
        lp = ft(0)
        for s in range(N):
            lp = lp + ft(theta[s, cfg[s]])
        for e in range(len(eu)):
            a, b = cfg[eu[e]], cfg[ev[e]]
            lp = lp - (ft(g[e]) * abs(ft(d[e]) - ft(b - a) * ft(dz)) if a < S and b < S else ft(0) if a == S and b == S else ft(switch))
        every.append(float(lp))
        if float(lp) > best:
            best, best_cfg = float(lp), cfg
        p = np.exp(lp)
        for s in range(N):
            marg[s, cfg[s]] += p
    return marg / marg.sum(axis=1, keepdims=True), np.array(best_cfg), best, np.array(every)


# ---- the rules where the answer is known ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("absent", [False, True])
def test_a_line_graph_is_the_chain(absent):
    rng = np.random.default_rng(10 + absent)
    N, S, dz, switch = 7, 9, 1.0, 2.5
    score, ab = rng.normal(size=(N, S)), (rng.normal(size=N) if absent else None)
    x, y, surface = np.cumsum(rng.uniform(5.0, 30.0, N)), np.zeros(N), rng.normal(size=N) * 2.0
    eu, ev = np.arange(N - 1), np.arange(1, N)
    g, d, dist = horizons.graph_steps(x, y, surface, eu, ev)
    gl, dl = horizons.steps(x, y, surface)
    assert np.array_equal(g, gl[:-1]) and np.array_equal(d, dl[:-1]) and np.array_equal(dist, np.diff(x))      # the steps of the line, bit for bit
    chain = horizons.track_reference([0, N], score, ab, gl, dl, dz, switch)
    chain_ld = horizons.track_reference([0, N], score, ab, gl, dl, dz, switch, dtype=np.longdouble)
    sweeps = N - 1                                                             # the diameter
    got = horizons.propagate_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=sweeps + 1)
    got_ld = horizons.propagate_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=sweeps + 1, dtype=np.longdouble)
    e = float(np.abs(got["belief"] - got_ld["belief"]).max())
    bound = 16.0 * max(e, U)
    dist_b = float(np.abs(got["belief"] - chain_ld["marginal"]).max())
    print("line absent=%s: e=%.3g used/bound %.3f" % (absent, e, dist_b / bound))
    assert got["belief"].dtype == np.float64 and got_ld["belief"].dtype == np.longdouble and got["state"].dtype == np.int32
    assert got["belief"].shape == (N, S + absent) and dist_b <= bound
    assert got["residual"].shape == (sweeps + 1,) and got["residual"][sweeps] == 0.0 and np.all(got["residual"][:3] > 0.0)
    path = horizons.graph_path_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=sweeps + 1)
    assert np.array_equal(path["decoded_state"], chain["cell"]) and np.array_equal(path["state"], chain["cell"]) and path["chosen"] == 0
    assert path["residual"][sweeps] == 0.0 and path["refine_moves"].sum() == 0 and np.all(path["max_marginal"].max(axis=1) == 0.0)
    assert abs(path["log_score"] - chain["log_score"][0]) <= 64 * U * max(1.0, abs(path["log_score"]))
    assert path["log_score"] == horizons.graph_log_score(chain["cell"], eu, ev, g, d, dz, switch, score, ab)
    few = horizons.graph_path_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=2, candidates=chain["cell"][None, :])
    assert few["log_score"] >= path["log_score"] and few["candidate_state"].shape == (2, N)      # never below a candidate given


def test_a_star_against_every_configuration():
    rng = np.random.default_rng(1)
    eu, ev, _ = star_graph()
    N, S, switch = 5, 3, 1.5
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, True, slope=0.8)
    want, mode, top, _ = brute_force(eu, ev, g, d, dz, switch, score, ab)
    got = horizons.propagate_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=4)
    dist = float(np.abs(got["belief"] - want).max())
    print("star: belief - marginal %.3g (bound 1e-12)" % dist)
    assert dist <= 1e-12
    assert got["residual"][3] == 0.0                                           # the diameter is 3 (1 - 0 - 3 - 4)
    path = horizons.graph_path_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=4)
    assert np.array_equal(path["state"], mode) and np.array_equal(path["decoded_state"], mode) and path["residual"][3] == 0.0
    assert abs(path["log_score"] - top) <= 64 * U * max(1.0, abs(top))
    none = np.zeros(0, dtype=np.int64)
    alone = horizons.propagate_reference(none, none, np.zeros(0), np.zeros(0), dz, switch, score, ab, sweeps=2)
    w = np.exp(np.concatenate([score, ab[:, None]], axis=1))
    assert np.allclose(alone["belief"], w / w.sum(axis=1, keepdims=True), rtol=0, atol=4 * U) and np.all(alone["residual"] == 0.0)
    apart = horizons.graph_path_reference(none, none, np.zeros(0), np.zeros(0), dz, switch, score, ab, sweeps=2)
    assert np.array_equal(apart["state"], np.argmax(np.concatenate([score, ab[:, None]], axis=1), axis=1))


def test_a_lattice_with_loops():
    """2 x 3 soundings, 3 cells and the absent state (two loops): the chosen log score lies between every candidate's and the enumerated
    maximum; the beliefs' distance from the exact marginals is the loop approximation DESIGN.md 3.33 records, printed and not held to
    a number."""
    rng = np.random.default_rng(2)
    eu, ev, N = lattice_graph(2, 3)
    S, switch = 3, 1.5
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, True, slope=0.8)
    want, mode, top, _ = brute_force(eu, ev, g, d, dz, switch, score, ab)
    got = horizons.propagate_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=40)
    print("lattice: residual", got["residual"][[0, 4, 9, 19, 39]], "belief - marginal %.3g" % float(np.abs(got["belief"] - want).max()))
    assert np.all(np.isfinite(got["belief"])) and float(np.abs(got["belief"].sum(axis=1) - 1.0).max()) <= 8 * U
    given = np.stack([got["state"], rng.integers(0, S + 1, N).astype(np.int32)])
    path = horizons.graph_path_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=40, candidates=given)
    print("lattice: chosen %d, log score %.6f, enumerated maximum %.6f, mode found: %s" % (path["chosen"], path["log_score"], top,
                                                                                          np.array_equal(path["state"], mode)))
    assert path["log_score"] <= top + 64 * U * max(1.0, abs(top))
    assert np.all(path["log_score"] >= path["candidate_log_score"]) and path["candidate_log_score"].shape == (3,)
    before = horizons.graph_log_score(np.concatenate([path["decoded_state"][None, :], given]), eu, ev, g, d, dz, switch, score, ab)
    assert np.all(path["candidate_log_score"] >= before)                       # the ascent never lowers a score
    assert path["log_score"] == horizons.graph_log_score(path["state"], eu, ev, g, d, dz, switch, score, ab)


def test_dyadic_ties_follow_the_stated_order():
    """Integer scores, g in {0.5, 1, 2}, d a multiple of dz = 0.5 and switch = 2: every sum is exact, so ties are ties."""
    eu, ev, N = lattice_graph(2, 3)
    S, dz, switch = 4, 0.5, 2.0
    rng = np.random.default_rng(5)
    score = rng.integers(-2, 3, (N, S)).astype(np.float64)
    ab = rng.integers(-2, 3, N).astype(np.float64)
    g, d = rng.choice([0.5, 1.0, 2.0], len(eu)), rng.integers(-3, 4, len(eu)) * dz
    path = horizons.graph_path_reference(eu, ev, g, d, dz, switch, score, ab, sweeps=12)
    _, mode, top, every = brute_force(eu, ev, g, d, dz, switch, score, ab)
    assert path["log_score"] <= top and np.all(path["max_marginal"].max(axis=1) == 0.0)
    assert path["log_score"] == every[int(np.ravel_multi_index(tuple(path["state"]), (S + 1,) * N))]      # exact arithmetic: not a bit away
    for s in range(N):                                                         # the first of equal max-marginals is the one at 0.0 first
        assert path["max_marginal"][s, int(np.argmax(path["max_marginal"][s]))] == 0.0
    # all-zero inputs: every configuration of cells at equal index ties with all-absent; the first maximum is cell 0, never absent
    zero = horizons.graph_path_reference(eu, ev, np.ones(len(eu)), np.zeros(len(eu)), dz, 0.0, np.zeros((N, S)), np.zeros(N), sweeps=6)
    assert np.all(zero["state"] == 0) and np.all(zero["decoded_state"] == 0) and zero["log_score"] == 0.0 and np.all(zero["max_marginal"][:, 0] == 0.0)
    ref =horizons.refine_reference(np.full(N, S), eu, ev, np.ones(len(eu)), np.zeros(len(eu)), dz, 0.0, np.zeros((N, S)), np.zeros(N))
    assert np.all(ref["state"] == S) and ref["refine_moves"].sum() == 0        # a tie moves nothing


def test_damping_zero_changes_no_bit():
    rng = np.random.default_rng(3)
    eu, ev, N = lattice_graph()
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, 5, True)
    for rule in (horizons.propagate_reference, horizons.graph_path_reference):
        plain, zero = rule(eu, ev, g, d, dz, 2.0, score, ab, sweeps=5), rule(eu, ev, g, d, dz, 2.0, score, ab, sweeps=5, damping=0.0)
        half = rule(eu, ev, g, d, dz, 2.0, score, ab, sweeps=5, damping=0.5)
        for name in plain:
            assert np.array_equal(np.asarray(plain[name]), np.asarray(zero[name])), name
        assert abs(half["residual"][0] - 0.5 * plain["residual"][0]) <= 8 * U * max(1.0, plain["residual"][0])


def test_a_zero_total_gives_nan():
    eu, ev, _ = star_graph()
    score, _, g, d, dz = horizon_inputs(np.random.default_rng(4), eu, ev, 5, 3, False)
    g[3], d[3] = 1e6, 0.3 * dz                                                 # every entry of the tail's K underflows: its messages are 0 / 0
    got = horizons.propagate_reference(eu, ev, g, d, dz, 2.0, score, None, sweeps=3)
    assert np.isnan(got["belief"][3]).all() and np.isnan(got["belief"][4]).all() and np.isnan(got["residual"]).all()
    assert np.isnan(got["belief"][0]).all() and got["state"][0] == 0           # the NaN travels; a NaN never replaces the first state
    path = horizons.graph_path_reference(eu, ev, g, d, dz, 2.0, score, None, sweeps=3)      # the log domain does not underflow
    assert np.all(np.isfinite(path["max_marginal"])) and np.isfinite(path["log_score"])


# ---- refusals, signatures -----------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_library():
    eu, ev, _ = star_graph()
    score, ab, g, d, dz = horizon_inputs(np.random.default_rng(6), eu, ev, 5, 3, True)
    t_score, t_ab = torch.as_tensor(score), torch.as_tensor(ab)
    rules = [lambda **kw: horizons.propagate_reference(**kw), lambda **kw: horizons.graph_path_reference(**kw),
             lambda **kw: horizons.propagate(**{**kw, "score": torch.as_tensor(kw["score"]), "absent_score": torch.as_tensor(kw["absent_score"])}),
             lambda **kw: horizons.graph_path(**{**kw, "score": torch.as_tensor(kw["score"]), "absent_score": torch.as_tensor(kw["absent_score"])})]
    base = dict(eu=eu, ev=ev, g=g, d=d, dz=dz, switch=2.0, score=score, absent_score=ab)
    for call in rules:
        for kw, match in ((dict(sweeps=0), "sweeps"), (dict(sweeps=1.5), "sweeps"), (dict(damping=1.0), "damping"), (dict(dz=0.0), "dz"),
                          (dict(switch=-1.0), "switch"), (dict(g=g[:-1]), "one entry per edge"), (dict(d=np.full(4, np.nan)), "finite"),
                          (dict(eu=ev, ev=eu), "eu < ev"), (dict(eu=eu[::-1], ev=ev[::-1]), "sorted"), (dict(absent_score=ab[:-1]), "absent_score"),
                          (dict(score=np.zeros((5, 0))), "score"), (dict(score=np.zeros((5, 2049)), absent_score=ab), "2048")):
            with pytest.raises(ValueError, match=match):
                call(**{**base, **kw})
    for call in rules[1::2]:
        for kw, match in ((dict(refine=-1), "refine"), (dict(candidates=np.zeros((1, 4), dtype=np.int64)), "candidates"),
                          (dict(candidates=np.full((1, 5), 4)), "0 .. 3"), (dict(candidates=np.zeros((1, 5))), "candidates")):
            with pytest.raises(ValueError, match=match):
                call(**{**base, **kw})
    with pytest.raises(ValueError, match="finite"):
        horizons.propagate_reference(**{**base, "score": np.full((5, 3), np.inf)})
    for call in (lambda s, **kw: horizons.refine(s, eu, ev, g, d, dz, 2.0, t_score, t_ab, **kw),
                 lambda s, **kw: horizons.refine_reference(s, eu, ev, g, d, dz, 2.0, score, ab, **kw)):
        with pytest.raises(ValueError, match="state"):
            call(np.zeros(4, dtype=np.int64))
        with pytest.raises(ValueError, match="0 .. 3"):
            call(np.array([0, 0, 4, 0, 0]))
        with pytest.raises(ValueError, match="sweeps"):
            call(np.zeros(5, dtype=np.int64), sweeps=-1)
    for call in (lambda: horizons.propagate(eu, ev, g, d, dz, 2.0, score, ab), lambda: horizons.graph_path(eu, ev, g, d, dz, 2.0, score, ab),
                 lambda: horizons.refine(np.zeros(5, dtype=np.int64), eu, ev, g, d, dz, 2.0, score, ab)):
        with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):     # numpy scores
            call()
    with pytest.raises(TypeError):
        horizons.propagate(eu, ev, g, d, dz, 2.0, t_score.float(), t_ab.float())
    for name, call in (("gbp_horizon_graph_propagate", lambda: horizons.propagate(eu, ev, g, d, dz, 2.0, t_score, t_ab)),
                       ("gbp_horizon_graph_path", lambda: horizons.graph_path(eu, ev, g, d, dz, 2.0, t_score, t_ab)),
                       ("gbp_horizon_graph_refine", lambda: horizons.refine(np.zeros(5, dtype=np.int64), eu, ev, g, d, dz, 2.0, t_score, t_ab))):
        with pytest.raises(_lib.NativeLibraryError, match=name):               # host tensors: refused last
            call()
    with pytest.raises(ValueError, match="graph_steps"):
        horizons.graph_steps(np.zeros(3), np.zeros(3), np.zeros(2), [0], [1])
    with pytest.raises(ValueError, match="slope"):
        horizons.graph_steps(np.zeros(3), np.zeros(3), np.zeros(3), [0], [1], slope=0.0)


def test_spatial_refuses_before_the_device():
    N, nz = 6, 8
    e, x, y, s, edges = torch.ones((N, nz), dtype=torch.float64), np.arange(N) * 10.0, np.zeros(N), np.zeros(N), np.arange(nz + 1.0)
    with pytest.raises(TypeError):
        horizons.spatial(e, x, y, s, edges)                                    # max_distance is required
    for kw, match in ((dict(sweeps=0), "sweeps"), (dict(damping=1.0), "damping"), (dict(between=(3.0, 1.0)), "between"), (dict(slope=0.0), "slope"),
                      (dict(message_budget_bytes=1000), "between="), (dict(percentiles=(0,)), "percentiles"), (dict(ptr=[0, 7]), "ptr")):
        with pytest.raises(ValueError, match=match):
            horizons.spatial(e, x, y, s, edges, max_distance=15.0, **kw)
    with pytest.raises(ValueError, match="between="):
        horizons.spatial(torch.ones((N, 2049), dtype=torch.float64), x, y, s, np.arange(2050.0), max_distance=15.0)
    assert horizons.message_bytes(5, 9) == 2 * 2 * 5 * 9 * 8
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        horizons.spatial(e, x, y, s, edges, max_distance=15.0)


def test_the_command_line_takes_spatial(capsys):
    base = ["a.h5", "b.h5", "--between", "10", "40"]
    a = horizons.parse_args(base + ["--spatial", "150"])
    assert a.spatial == 150.0 and a.sweeps == 32 and a.damping == 0.0 and not a.no_path
    a = horizons.parse_args(base + ["--spatial", "150", "--sweeps", "12", "--damping", "0.25", "--no-path"])
    assert a.sweeps == 12 and a.damping == 0.25 and a.no_path
    assert horizons.parse_args(base).spatial is None                           # without --spatial nothing changes
    for argv in (base + ["--sweeps", "12"], base + ["--no-path"], base + ["--damping", "0.5"], base + ["--spatial", "0"],
                 base + ["--spatial", "150", "--sweeps", "0"], base + ["--spatial", "150", "--damping", "1"]):
        with pytest.raises(SystemExit):
            horizons.parse_args(argv)
    capsys.readouterr()


def test_the_signatures_declare_the_entries():
    counts = (("gbp_horizon_graph_propagate", 22), ("gbp_horizon_graph_path", 25), ("gbp_horizon_graph_refine", 21))
    with open(os.path.join(ROOT, "include", "geobipy_amd.h")) as f:
        text = f.read()
    for name, count in counts:
        assert len(_lib.SIGNATURES[name][1]) == count, name
        declaration = text.split("gbp_status %s(" % name)[1].split(");")[0]
        assert len(declaration.split(",")) == count, name
    with open(os.path.join(ROOT, "geobipy_amd", "csrc", "gbp_fdem.hip")) as f:
        lines = [line.strip() for line in f if line.startswith("#include \"gbp_")]
    assert lines.index('#include "gbp_horizon_graph.h"') > lines.index('#include "gbp_section_graph_path.h"')
    from geobipy_amd import build
    assert "gbp_horizon_graph.h" in build.HEADERS


# ---- the planted lines ----------------------------------------------------------------------------------------------------------------

LINES, PER_LINE, CELLS, DECOY_CELLS = 3, 12, 64, 11


def planted_horizon():
    """3 lines x 12 soundings, x = 50 i, y = 100 line, on a tilted surface over a tilted horizon; the middle line carries a stronger
    decoy eleven cells deeper along its whole length.  Returns evidence [36, 64], x, y, surface, depth_edges, ptr, the planted cells."""
    i, line = np.tile(np.arange(PER_LINE), LINES), np.repeat(np.arange(LINES), PER_LINE)
    x, y = 50.0 * i, 100.0 * line
    surface = 0.01 * x + 0.02 * y
    depth = surface - (-12.0 - 0.02 * x - 0.01 * y)
    cell = np.floor(depth / 1.0).astype(np.int64)
    evidence = np.full((LINES * PER_LINE, CELLS), 0.02)
    evidence[np.arange(cell.size), cell] += 1.0
    middle = np.flatnonzero(line == 1)
    evidence[middle, cell[middle] + DECOY_CELLS] += 1.6
    return evidence, x, y, surface, np.arange(CELLS + 1.0), np.arange(LINES + 1) * PER_LINE, cell


def test_the_planted_lines_on_the_rules_alone():
    evidence, x, y, surface, edges, ptr, cell = planted_horizon()
    middle = np.arange(PER_LINE, 2 * PER_LINE)
    score, _ = horizons.evidence_scores(evidence)
    gl, dl = horizons.steps(x, y, surface, ptr=ptr)
    alone = horizons.track_reference(ptr, score, None, gl, dl, 1.0, 4.6, marginals=False)["cell"]
    assert np.array_equal(alone[middle], cell[middle] + DECOY_CELLS)           # 12 of 12 on the decoy
    assert np.array_equal(np.delete(alone, middle), np.delete(cell, middle))
    eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=150.0)
    assert eu.size == 57
    g, d, _ = horizons.graph_steps(x, y, surface, eu, ev)
    found = horizons.propagate_reference(eu, ev, g, d, 1.0, 4.6, score, None, sweeps=16)
    path = horizons.graph_path_reference(eu, ev, g, d, 1.0, 4.6, score, None, sweeps=16, candidates=np.stack([found["state"], alone]))
    assert np.array_equal(found["state"], cell)                                # 36 of 36 on the planted horizon
    assert np.array_equal(path["decoded_state"], cell) and np.array_equal(path["state"], cell)
    assert path["log_score"] > path["candidate_log_score"][2] and path["candidate_log_score"][2] >= horizons.graph_log_score(alone, eu, ev, g, d, 1.0, 4.6, score)
