"""The evidence of the lateral coupling tau along lines, on the rules alone (geobipy_amd.sections evidence_reference,
evidence_reference_ladder, fit_tau_reference).  No device is touched.

``evidence_reference`` is held to the enumeration of every path of small chains (log Z and -E[cost], within 1e-13), to
``track_reference`` at rung 0, to the central difference of its own long-double log Z in lambda, and its squared ladder to a direct
exp.  ``fit_tau_reference`` is held to the exact answer of a one-parameter model: the maximiser of the Kalman likelihood of a random
walk observed in noise, within two of the fit's own standard errors."""
import itertools

import numpy as np
import pytest

from geobipy_amd import sections
from test_spatial_sections import graph_inputs, lattice_graph, line_graph, star_graph

LD = np.longdouble


def small_chain(seed, counts, n, with_score, spread=1.0):
    """A chain of len(counts) soundings with n states of which counts[s] are used: (ptr, score or None, g, d2, n_used); NaN outside
    the prefixes of d2 and score, so that a read outside them shows."""
    rng = np.random.default_rng(seed)
    total = len(counts)
    nu = np.asarray(counts, dtype=np.int32)
    d2 = np.full((total, n, n), np.nan)
    score = np.full((total, n), np.nan) if with_score else None
    for s in range(total):
        if s + 1 < total:
            d2[s, :nu[s], :nu[s + 1]] = spread * rng.random((nu[s], nu[s + 1])) ** 2
        if with_score:
            score[s, :nu[s]] = rng.normal(0.0, 1.0, nu[s])
    g = rng.uniform(0.5, 3.0, total)
    return np.array([0, total], dtype=np.int64), score, g, d2, nu


def enumerate_chain(score, g, d2, nu, c):
    """(ln Z, -E[cost]) of one sequence at scale c by the sum over every path, in long double."""
    total = nu.size
    Z, ZC = LD(0), LD(0)
    for path in itertools.product(*[range(int(m)) for m in nu]):
        cost = sum((LD(c) * LD(g[s]) * LD(d2[s, path[s], path[s + 1]]) for s in range(total - 1)), LD(0))
        lw = sum((LD(score[s, path[s]]) for s in range(total)), LD(0)) if score is not None else LD(0)
        p = np.exp(lw - cost)
        Z, ZC = Z + p, ZC + p * cost
    return np.log(Z), -ZC / Z


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("with_score", [False, True])
@pytest.mark.parametrize("counts,n", [((3, 1, 4, 2, 4), 4), ((2, 3), 3), ((4, 4, 4, 4), 4), ((1, 1, 1), 2)])
def test_rule_against_the_enumeration_of_every_path(counts, n, with_score, dtype):
    ptr, score, g, d2, nu = small_chain(len(counts) * 10 + n, counts, n, with_score)
    out = sections.evidence_reference(ptr, score, g, d2, nu, T=3, dtype=dtype)
    assert out["log_partition"].shape == (3, 1) and out["dlog_partition"].shape == (3, 1) and out["log_partition"].dtype == np.dtype(dtype)
    worst = 0.0
    for t in range(3):
        lz, dlz = enumerate_chain(score, g, d2, nu, 2.0 ** t)
        worst = max(worst, abs(float(out["log_partition"][t, 0] - lz)), abs(float(out["dlog_partition"][t, 0] - dlz)))
    print("rule - enumeration: %.3g" % worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("with_score", [False, True])
def test_rung_zero_is_the_log_partition_of_track(with_score):
    ptr, score, g, d2, nu = small_chain(5, (3, 5, 1, 4, 5, 2, 5), 5, with_score)
    ptr = np.array([0, 3, 4, 7], dtype=np.int64)                              # three sequences, one of a single sounding
    got = sections.evidence_reference(ptr, score, g, np.nan_to_num(d2), nu, T=2)
    want = sections.track_reference(ptr, score if score is None else np.nan_to_num(score), g, np.nan_to_num(d2), nu)["log_partition"]
    assert np.max(np.abs(got["log_partition"][0] - want)) <= 1e-13
    twice = sections.track_reference(ptr, score if score is None else np.nan_to_num(score), 2.0 * g, np.nan_to_num(d2), nu)["log_partition"]
    assert np.max(np.abs(got["log_partition"][1] - twice)) <= 1e-13
    w1 = np.log(nu[3]) if score is None else np.log(np.exp(score[3, :nu[3]]).sum())
    assert abs(got["log_partition"][0, 1] - w1) <= 1e-15 and np.all(got["dlog_partition"][:, 1] == 0.0)      # one sounding: ln sum w and 0.0


def test_derivative_against_the_central_difference():
    """h = 1e-4 in lambda: the difference's own error is h^2 / 6 |d^3 log Z / d lambda^3| (about 1e-9 times a value of the size of
    log Z's derivatives here) beside long double's rounding 1e-19 / h; the bar is 1e-6 of max(1, |value|)."""
    ptr, score, g, d2, nu = small_chain(11, (4, 3, 5, 5, 2, 5), 5, True)
    h = 1e-4
    out = sections.evidence_reference(ptr, score, g, d2, nu, T=4, dtype=LD)
    for t in range(4):
        up = sections.evidence_reference(ptr, score, g * (2.0 ** t * np.exp(h)), d2, nu, T=1, dtype=LD)["log_partition"][0, 0]
        dn = sections.evidence_reference(ptr, score, g * (2.0 ** t * np.exp(-h)), d2, nu, T=1, dtype=LD)["log_partition"][0, 0]
        diff, got = float((up - dn) / (2 * h)), float(out["dlog_partition"][t, 0])
        assert got < 0.0 and abs(got - diff) <= 1e-6 * max(1.0, abs(got)), (t, got, diff)


def test_the_squared_ladder_against_a_direct_exp():
    ptr, score, g, d2, nu = small_chain(3, (5, 5, 4, 5, 5, 3), 5, True, spread=0.05)
    top = sections.evidence_reference(ptr, score, g, d2, nu, T=8, dtype=LD)
    direct = sections.evidence_reference(ptr, score, 128.0 * g, d2, nu, T=1, dtype=LD)
    for name in ("log_partition", "dlog_partition"):
        a, b = top[name][7, 0], direct[name][0, 0]
        assert abs(a - b) <= 1e-15 * abs(b), (name, float(a), float(b))


def test_no_sequence_and_empty_sequences():
    none = sections.evidence_reference(np.array([0]), None, np.zeros(0), np.zeros((0, 3, 3)), np.zeros(0, dtype=np.int32), T=2)
    assert none["log_partition"].shape == (2, 0) and none["dlog_partition"].shape == (2, 0)
    lad = sections.evidence_reference_ladder(np.zeros((0, 3, 3)), np.zeros(0), np.array([0]), np.zeros(0, dtype=np.int32), rungs=3)
    assert lad["log_evidence"].shape == (3, 0) and lad["rank"].size == 0 and lad["tau"].shape == (3,)


def underflow_chain():
    """Three soundings; every cost of the second step lies in 250 .. 300 at rung 0: above 800 from rung 2 on, where exp gives 0.0."""
    ptr, score, g, d2, nu = small_chain(2, (3, 4, 3), 4, True)
    g[:] = 1.0
    d2[1, :4, :3] = 250.0 + 50.0 * np.random.default_rng(4).random((4, 3))
    return ptr, score, g, d2, nu


def test_a_rung_that_underflows_is_not_finite_and_leaves_the_rungs_below_alone():
    ptr, score, g, d2, nu = underflow_chain()
    out = sections.evidence_reference(ptr, score, g, d2, nu, T=4)
    below = sections.evidence_reference(ptr, score, g, d2, nu, T=2)
    for name in ("log_partition", "dlog_partition"):
        assert np.all(np.isfinite(out[name][:2])) and not np.any(np.isfinite(out[name][2:])), name
        assert np.array_equal(out[name][:2], below[name])


def test_rank_and_the_log_evidence():
    ptr, score, g, d2, nu = small_chain(8, (3, 2, 4, 4, 1, 3), 4, True)
    ptr = np.array([0, 3, 3, 4, 6], dtype=np.int64)                           # 3 soundings, none, 1, 2
    lad = sections.evidence_reference_ladder(np.nan_to_num(d2), g, ptr, nu, score=np.nan_to_num(score), tau0=0.2, rungs=3, scale=0.5)
    assert np.array_equal(lad["rank"], [2, 0, 0, 1])                          # soundings minus sequences that hold any
    assert np.allclose(lad["scale"], [0.5, 1.0, 2.0]) and np.allclose(lad["tau"], 0.2 / np.sqrt([0.5, 1.0, 2.0]))
    log_w = np.array([np.log(np.exp(score[s, :nu[s]]).sum()) for s in range(6)])
    base = np.array([log_w[:3].sum(), 0.0, log_w[3], log_w[4:].sum()])
    want = lad["log_partition"] + 0.5 * lad["rank"][None, :] * np.log(lad["scale"])[:, None] - base[None, :]
    assert np.max(np.abs(lad["log_evidence"] - want)) <= 1e-13
    assert np.all(lad["log_evidence"][:, 1] == 0.0) and np.max(np.abs(lad["log_evidence"][:, 2])) <= 1e-15      # nothing to learn from them


def test_the_ladder_is_split_where_it_does_not_fit_a_launch():
    assert sections.ladder_launches(64, 11) == [(0, 8), (8, 3)]
    assert sections.ladder_launches(256, 8) == [(0, 8)] and sections.ladder_launches(257, 8) == [(0, 7), (7, 1)]
    assert sections.ladder_launches(1024, 3) == [(0, 2), (2, 1)] and sections.ladder_launches(1, 1) == [(0, 1)]
    ptr, score, g, d2, nu = small_chain(9, (3, 3, 3, 3), 3, False)
    lad = sections.evidence_reference_ladder(d2, g, ptr, nu, rungs=10)
    tail = sections.evidence_reference(ptr, None, g * 2.0 ** 8, d2, nu, T=2)   # the second launch takes its own exp
    assert np.array_equal(lad["log_partition"][8:], tail["log_partition"]) and np.array_equal(lad["dlog_partition"][8:], tail["dlog_partition"])


# ---- the fit against the Kalman likelihood ------------------------------------------------------------------------------------------

WALK = dict(N=200, dx=25.0, sd=0.05, tau_true=0.1, length=100.0)


def planted_walk(seed, n=64):
    """N soundings 25 m apart on one line; a one-parameter model per sounding: the truth is a random walk of ``tau_true`` decades per
    100 m, y_s the truth in noise of ``sd``, and the kept models of sounding s are y_s + N(0, sd^2): draws of its posterior under a flat
    prior.  Returns y, x, ptr, g at tau0 = 0.1, d2 [N, n, n] and n_used."""
    rng = np.random.default_rng(seed)
    N, dx, sd = WALK["N"], WALK["dx"], WALK["sd"]
    truth = np.cumsum(rng.normal(0.0, WALK["tau_true"] * np.sqrt(dx / WALK["length"]), N))
    y = truth + rng.normal(0.0, sd, N)
    models = y[:, None] + rng.normal(0.0, sd, (N, n))
    d2 = np.zeros((N, n, n))
    d2[:-1] = (models[:-1, :, None] - models[1:, None, :]) ** 2
    x = dx * np.arange(N)
    return y, x, np.array([0, N], dtype=np.int64), sections.steps(x, np.zeros(N), tau=0.1, length=WALK["length"]), d2, np.full(N, n, dtype=np.int32)


def kalman_tau(y):
    """The maximiser over a 600-point grid of tau of the exact likelihood of y: a random walk of variance tau^2 dx / length per step,
    observed in noise of sd, started from the first observation (a flat prior on the first value)."""
    taus = np.geomspace(0.02, 0.5, 600)
    v, r = taus ** 2 * WALK["dx"] / WALK["length"], WALK["sd"] ** 2
    mean, P, ll = np.full(taus.size, y[0]), np.full(taus.size, r), np.zeros(taus.size)
    for obs in y[1:]:
        Pp = P + v
        S = Pp + r
        ll += -0.5 * (np.log(2 * np.pi * S) + (obs - mean) ** 2 / S)
        K = Pp / S
        mean, P = mean + K * (obs - mean), (1.0 - K) * Pp
    return float(taus[np.argmax(ll)])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_against_the_kalman_maximiser(seed):
    """The bar is the fit's own standard error, twice."""
    y, x, ptr, g, d2, nu = planted_walk(seed)
    fit = sections.fit_tau_reference(d2, g, ptr, nu)
    tau_k = kalman_tau(y)
    print("seed %d: tau_hat %.4f  kalman %.4f  |ln ratio| %.3f  sd_log %.3f  bracket %r  evaluations %d"
          % (seed, fit["tau"], tau_k, abs(np.log(fit["tau"] / tau_k)), fit["tau_sd_log"], fit["bracket"], fit["evaluations"]))
    assert fit["bracketed"] and fit["rank"] == WALK["N"] - 1 and fit["evaluations"] <= sections.FIT_EVALUATIONS
    assert fit["tau_ladder"].shape == (11,) and abs(fit["tau_ladder"][0] - 0.8) < 1e-15 and abs(fit["tau_ladder"][-1] - 0.025) < 1e-15
    assert fit["log_evidence"].shape == (11,) and fit["log_evidence_sequence"].shape == (11, 1) and fit["expected_cost"].shape == (11,)
    lo, hi = fit["bracket"]
    assert hi == lo + 1 and fit["tau_ladder"][hi] <= fit["tau"] <= fit["tau_ladder"][lo]
    assert abs(int(np.argmax(fit["log_evidence"])) - lo) <= 1                 # the evidence peaks where its derivative changes sign
    assert abs(np.log(fit["tau"] / tau_k)) <= 2.0 * fit["tau_sd_log"]


def test_a_ladder_that_ends_too_high_has_no_bracket():
    y, x, ptr, g, d2, nu = planted_walk(0, n=16)
    fit = sections.fit_tau_reference(d2, g, ptr, nu, tau_max=0.8, rungs=3)    # 0.8, 0.57, 0.4: all looser than the data ask for
    assert fit["bracketed"] is False and fit["bracket"] == (-1, -1) and np.isnan(fit["tau_sd_log"]) and fit["evaluations"] == 0
    assert abs(fit["tau"] - 0.4) < 1e-12
    low = sections.fit_tau_reference(d2, g, ptr, nu, tau_max=0.01, rungs=2)   # all stiffer: the ladder's upper end
    assert low["bracketed"] is False and abs(low["tau"] - 0.01) < 1e-15


# ---- the survey graph: the Bethe evidence --------------------------------------------------------------------------------------------

def enumerate_graph(eu, ev, g, d2, nu, score, c=1.0):
    """(ln Z, -E[cost]) of the graph at scale c by the sum over every configuration, in long double."""
    Z, ZC = LD(0), LD(0)
    for cfg in itertools.product(*[range(int(m)) for m in nu]):
        cost = sum((LD(c) * LD(g[e]) * LD(d2[e, cfg[eu[e]], cfg[ev[e]]]) for e in range(len(eu))), LD(0))
        lw = sum((LD(score[s, cfg[s]]) for s in range(len(nu))), LD(0)) if score is not None else LD(0)
        p = np.exp(lw - cost)
        Z, ZC = Z + p, ZC + p * cost
    return float(np.log(Z)), float(-ZC / Z)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_bethe_evidence_is_exact_on_a_tree(dtype):
    rng = np.random.default_rng(21)
    eu, ev, nu = star_graph()                                                  # diameter 3
    score, g, d2 = graph_inputs(rng, eu, ev, nu, 3)
    for scale in (1.0, 0.25):
        got = sections.graph_evidence_reference(eu, ev, g, d2, nu, score, scale=scale, sweeps=4, dtype=dtype)
        lz, dlz = enumerate_graph(eu, ev, g, d2, nu, score, scale)
        print("tree: log Z %.3g dlog Z %.3g" % (abs(got["log_partition"] - lz), abs(got["dlog_partition"] - dlz)))
        assert abs(got["log_partition"] - lz) <= 1e-12 and abs(got["dlog_partition"] - dlz) <= 1e-12
        assert got["rank"] == 4 and got["residual"][-1] == 0.0 and got["edge_energy"].shape == (4,) and np.all(got["edge_energy"] > 0.0)
        log_w = sum(np.log(np.exp(score[s, :nu[s]]).sum()) for s in range(5))
        assert abs(got["log_evidence"] - (got["log_partition"] + 2.0 * np.log(scale) - log_w)) <= 1e-12


def test_bethe_evidence_of_a_line_is_the_chain_evidence():
    rng = np.random.default_rng(22)
    eu, ev, nu = line_graph()
    score, g, d2 = graph_inputs(rng, eu, ev, nu, 5)
    S = nu.size
    chain = sections.evidence_reference([0, S], score, np.append(g, 1.0), np.concatenate([d2, np.zeros((1, 5, 5))]), nu, T=2)
    for t, scale in enumerate((1.0, 2.0)):
        got = sections.graph_evidence_reference(eu, ev, g, d2, nu, score, scale=scale, sweeps=5)
        assert abs(got["log_partition"] - chain["log_partition"][t, 0]) <= 1e-12
        assert abs(got["dlog_partition"] - chain["dlog_partition"][t, 0]) <= 1e-12


# what graph_evidence_reference gave against the enumeration when this test was written (DESIGN.md 3.35 records them): the loop
# approximation of the Bethe evidence on a 3 x 3 lattice of 3 states, as (gap of log Z_B, gap of dlog Z_B) at a quarter of the
# couplings of graph_inputs and, four times as stiff, at those couplings themselves; the test allows twice as much
LATTICE_GAP = {0.25: (6.584e-4, 5.125e-4), 1.0: (1.760e-3, 3.812e-3)}


@pytest.mark.parametrize("scale", [0.25, 1.0])
def test_bethe_evidence_on_loops_stays_within_twice_its_recorded_gap(scale):
    rng = np.random.default_rng(23)
    eu, ev, S = lattice_graph(3, 3)
    nu = np.full(S, 3)
    score, g, d2 = graph_inputs(rng, eu, ev, nu, 3)
    got = sections.graph_evidence_reference(eu, ev, g, d2, nu, score, scale=scale, sweeps=200)
    lz, dlz = enumerate_graph(eu, ev, g, d2, nu, score, scale)
    gap = abs(got["log_partition"] - lz), abs(got["dlog_partition"] - dlz)
    print("lattice scale %g: residual %.3g, gap of log Z %.4g, of dlog Z %.4g" % (scale, got["residual"][-1], gap[0], gap[1]))
    assert got["residual"][-1] < 1e-12 and got["rank"] == 8                    # 12 edges, 4 loops
    assert 0.0 < gap[0] <= 2.0 * LATTICE_GAP[scale][0] and 0.0 < gap[1] <= 2.0 * LATTICE_GAP[scale][1]


def test_rank_of_a_graph():
    eu, ev, S = lattice_graph(3, 3)
    assert sections.graph_rank(eu, ev, S) == 8
    tree_eu, tree_ev, nu = star_graph()
    assert sections.graph_rank(tree_eu, tree_ev, 5) == 4
    assert sections.graph_rank([0, 0, 1], [1, 2, 2], 3) == 2                   # a loop adds an edge and no rank
    assert sections.graph_rank([0, 0, 1, 3], [1, 2, 2, 4], 6) == 3             # two more components (3 - 4, and 5 alone) subtract two
    assert sections.graph_rank([], [], 4) == 0 and sections.graph_rank([], [], 0) == 0


def test_fit_on_a_line_graph_is_the_fit_on_the_chain():
    y, x, ptr, g, d2, nu = planted_walk(0, n=8)
    N = 30                                                                     # the first 30 soundings: a tree of diameter 29
    ptr, g, d2, nu = np.array([0, N]), g[:N], d2[:N], nu[:N]
    chain = sections.fit_tau_reference(d2, g, ptr, nu)
    graph = sections.fit_tau_graph_reference(np.arange(N - 1), np.arange(1, N), g[:-1], d2[:-1], nu, sweeps=N)
    assert graph["bracketed"] and graph["bracket"] == chain["bracket"] and graph["rank"] == N - 1
    assert abs(np.log(graph["tau"] / chain["tau"])) <= 1e-9 and abs(graph["tau_sd_log"] - chain["tau_sd_log"]) <= 1e-6
    assert graph["residual"].shape == (11,) and np.all(graph["residual"] == 0.0) and graph["log_evidence_sequence"].shape == (11, 1)
    assert np.allclose(graph["log_evidence"], chain["log_evidence"], rtol=0, atol=1e-9)


def test_the_parser(capsys):
    path, kw = sections.parse_args(["s.npz", "--depth", "120"])
    assert kw["tau"] == 0.1 and "fit_tau" not in kw                            # without --fit-tau nothing changes
    assert sections.parse_args(["s.npz", "--depth", "120", "--tau", "0.3"])[1]["tau"] == 0.3
    assert sections.parse_args(["s.npz", "--depth", "120", "--fit-tau"])[1]["fit_tau"] == dict(tau_max=0.8, rungs=11)
    assert sections.parse_args(["s.npz", "--depth", "120", "--fit-tau", "0.4"])[1]["fit_tau"] == dict(tau_max=0.4, rungs=11)
    both = sections.parse_args(["s.npz", "--depth", "120", "--fit-tau", "0.4", "7", "--spatial", "150", "--max-models", "64"])[1]
    assert both["fit_tau"] == dict(tau_max=0.4, rungs=7) and both["max_distance"] == 150.0 and both["tau"] == 0.1
    for argv, message in ((["--fit-tau", "--tau", "0.2"], "not given together with --tau"), (["--tau", "0.2", "--fit-tau", "0.8"], "not given together with --tau"),
                          (["--fit-tau", "0.8", "1"], "rungs"), (["--fit-tau", "0"], "tau_max"), (["--fit-tau", "0.8", "2.5"], "a number and an integer"),
                          (["--fit-tau", "0.8", "5", "7"], "a number and an integer")):
        with pytest.raises(SystemExit):
            sections.parse_args(["s.npz", "--depth", "120"] + argv)
        assert message in capsys.readouterr().err, argv


def test_refusals():
    ptr, score, g, d2, nu = small_chain(1, (2, 2), 2, False)
    for T in (0, 9, 1.5, True):
        with pytest.raises((ValueError, TypeError), match="T"):
            sections.evidence_reference(ptr, None, g, d2, nu, T=T)
    with pytest.raises(ValueError, match="n_used must lie in 1 .. n"):
        sections.evidence_reference(ptr, None, g, d2, [2, 3], T=1)
    with pytest.raises(ValueError, match="g must hold one entry per sounding"):
        sections.evidence_reference(ptr, None, g[:1], d2, nu, T=1)
    with pytest.raises(ValueError, match=r"score must be \[T, n\]"):
        sections.evidence_reference(ptr, np.zeros((2, 3)), g, d2, nu, T=1)
    for kw, what in ((dict(tau0=0.0), "tau0"), (dict(tau0=np.nan), "tau0"), (dict(scale=-1.0), "scale"), (dict(rungs=0), "rungs"), (dict(rungs=65), "rungs")):
        with pytest.raises((ValueError, TypeError), match=what):
            sections.evidence_reference_ladder(d2, g, ptr, nu, **kw)
    for kw, what in ((dict(tau_max=0.0), "tau_max"), (dict(tau_max="a"), "tau_max"), (dict(rungs=1), "rungs"), (dict(tau0=-0.1), "tau0")):
        with pytest.raises((ValueError, TypeError), match=what):
            sections.fit_tau_reference(d2, g, ptr, nu, **kw)
