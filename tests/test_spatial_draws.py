"""Joint draws across flight lines, the rules alone (geobipy_amd.sections graph_draw_reference, line_colours): no GPU.

Line-blocked Gibbs sampling is held to what it must equal where that is known: ``draw_reference`` bit for bit without cross edges, the
smoothed marginals of a chain, and the exact joint of a small graph WITH loops by enumeration in long double -- where the beliefs of
3.28 are only an approximation.  The statistical bound is that of test_section_draws.py: every compared cell within 5 standard
deviations of its binomial count, seeds fixed, every case prints its worst |z|."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, sections
from test_section_draws import R_STAT, check_marginal_frequencies, ragged_chain, worst_z
from test_spatial_sections import (S_LINES, SPACING, Z1_LINES, brute_force, edge_distance_reference, graph_inputs, lattice_graph, planted_lines,
                                   star_graph)

LADDER_SWEEPS = 6                                                              # T of the ladder: the rule passes at T and at 2 T (checked on the CPU)
LADDER_SEED = 17


def chain_as_graph(ptr, g, d2, n_used):
    """The edges of the chains of ``ptr``: (eu, ev, g [E], d2 [E, n, n]) from the per-sounding arrays of ``draw_reference``."""
    ptr = np.asarray(ptr)
    last = np.zeros(len(n_used), dtype=bool)
    last[ptr[1:][np.diff(ptr) > 0] - 1] = True
    eu = np.flatnonzero(~last)
    return eu, eu + 1, np.asarray(g)[eu], np.asarray(d2)[eu]


def ladder_case():
    """Two lines of three soundings and three cross edges (two loops): ragged n_used <= 3 with one single state, random scores, g d2 of
    order 1 -- and cross couplings strong enough that the line-alone start is far from the joint.  Returns (eu, ev, g, d2, n_used,
    score, ptr)."""
    rng = np.random.default_rng(23)
    eu, ev = np.array([0, 0, 1, 1, 2, 3, 4]), np.array([1, 3, 2, 4, 5, 4, 5])
    n_used = np.array([3, 2, 3, 3, 1, 3])
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 3)
    g = rng.uniform(2.0, 6.0, eu.size)
    d2 = np.where(np.isnan(d2), d2, rng.uniform(0.0, 0.8, d2.shape))
    return eu, ev, g, d2, n_used, score, np.array([0, 3, 6])


def exact_joint(eu, ev, g, d2, n_used, score):
    """The exact joint of the graph by enumeration in long double: (configurations, their probabilities)."""
    ld = np.longdouble
    cfgs = list(itertools.product(*[range(int(m)) for m in n_used]))
    lw = np.array([sum(ld(score[s, c[s]]) for s in range(len(n_used))) - sum(ld(g[e]) * ld(d2[e, c[eu[e]], c[ev[e]]]) for e in range(len(eu))) for c in cfgs])
    p = np.exp(lw - lw.max())
    return np.array(cfgs), (p / p.sum()).astype(np.float64)


def exact_marginals(cfgs, prob, n):
    out = np.zeros((cfgs.shape[1], n))
    for s in range(cfgs.shape[1]):
        np.add.at(out[s], cfgs[:, s], prob)
    return out


def marginal_z(draw_state, marginal, R, least=8):
    counts = np.stack([np.bincount(draw_state[:, s], minlength=marginal.shape[1]) for s in range(marginal.shape[0])])
    return worst_z(counts, marginal, R, least)[0]


def check_ladder(draw_state, what, R=R_STAT):
    """The per-sounding frequencies against the exact marginals and the joint frequencies of the ends of the cross edge (1, 4) -- and
    of (0, 3) -- against the exact pair marginals, within 5 sigma on the cells of expected count >= 30."""
    eu, ev, g, d2, n_used, score, _ = ladder_case()
    cfgs, prob = exact_joint(eu, ev, g, d2, n_used, score)
    assert len(cfgs) <= 729
    z = marginal_z(draw_state, exact_marginals(cfgs, prob, 3), R)
    worst_pair = 0.0
    for a, b in ((0, 3), (1, 4)):
        pair = np.zeros((3, 3))
        np.add.at(pair, (cfgs[:, a], cfgs[:, b]), prob)
        counts = np.zeros((3, 3))
        np.add.at(counts, (draw_state[:, a], draw_state[:, b]), 1.0)
        cells = (R * pair >= 30.0) & (pair < 1.0)
        assert cells.sum() >= 2
        worst_pair = max(worst_pair, float((np.abs(counts[cells] - R * pair[cells]) / np.sqrt(R * pair[cells] * (1.0 - pair[cells]))).max()))
    print("%s: worst |z| of the marginals %.2f, of the pairs %.2f" % (what, z, worst_pair))
    assert np.all(draw_state < n_used[None, :]) and np.all(draw_state >= 0)
    assert z <= 5.0 and worst_pair <= 5.0


# ---- without cross edges the scheme is the draws of 3.26 --------------------------------------------------------------------------------

def test_without_cross_edges_the_start_is_draw_reference_and_sweeps_keep_the_marginals():
    ptr, score, g, d2, n_used = ragged_chain(21, 6, 12)
    eu, ev, ge, de = chain_as_graph(ptr, g, d2, n_used)
    key = (np.arange(12) * 7 + 2 ** 33).astype(np.int64)
    want = sections.draw_reference(ptr, score, g, d2, n_used, R_STAT, seed=3, row_key=key)
    got = sections.graph_draw_reference(eu, ev, ge, de, n_used, ptr, R_STAT, seed=3, sweeps=0, score=score, row_key=key)
    assert got["draw_state"].dtype == np.int32 and np.array_equal(got["draw_state"], want["draw_state"])
    assert np.array_equal(got["margin"], want["margin"]) and np.array_equal(got["filtered"][5], want["filtered"])
    ld = sections.track_reference(ptr, score, g, d2, n_used, dtype=np.longdouble)["marginal"].astype(np.float64)
    three = sections.graph_draw_reference(eu, ev, ge, de, n_used, ptr, R_STAT, seed=3, sweeps=3, score=score, row_key=key)
    assert not np.array_equal(three["draw_state"], want["draw_state"])          # the sweep goes into the random numbers
    check_marginal_frequencies(three["draw_state"], ld, n_used, R_STAT, "one ragged line, 3 sweeps")
    assert three["filtered"].shape == (R_STAT, 12, 6) and np.all(three["margin"] <= want["margin"])

    # three lines out of each other's reach, one of them a single sounding, and an empty sequence
    ptr3 = np.array([0, 5, 5, 6, 12])
    eu, ev, ge, de = chain_as_graph(ptr3, g, d2, n_used)
    want = sections.draw_reference(ptr3, score, g, d2, n_used, 300, seed=8)
    got = sections.graph_draw_reference(eu, ev, ge, de, n_used, ptr3, 300, seed=8, sweeps=0, score=score)
    assert np.array_equal(got["draw_state"], want["draw_state"]) and np.array_equal(got["margin"], want["margin"])
    colour, n_colours = sections.line_colours(eu, ev, ptr3)
    assert colour.tolist() == [0, 0, 0, 0] and n_colours == 1
    lines = sections.graph_draw_reference(eu, ev, ge, de, n_used, ptr3, R_STAT, seed=8, sweeps=3, score=score)
    ld = sections.track_reference(ptr3[[0, 1, 3, 4]], score, g, d2, n_used, dtype=np.longdouble)["marginal"].astype(np.float64)
    check_marginal_frequencies(lines["draw_state"], ld, n_used, R_STAT, "three lines apart, 3 sweeps")


# ---- the exact law with loops -----------------------------------------------------------------------------------------------------------

def test_the_ladder_reaches_the_exact_joint_and_the_start_does_not():
    eu, ev, g, d2, n_used, score, ptr = ladder_case()
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    assert colour.tolist() == [0, 1] and n_colours == 2
    cfgs, prob = exact_joint(eu, ev, g, d2, n_used, score)
    start = sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R_STAT, seed=LADDER_SEED, sweeps=0, score=score)
    z0 = marginal_z(start["draw_state"], exact_marginals(cfgs, prob, 3), R_STAT)
    print("ladder: the line-alone start misses the exact marginals by |z| = %.1f" % z0)
    assert z0 > 10.0                                                           # a scheme that ignores the cross edges is seen
    for T in (LADDER_SWEEPS, 2 * LADDER_SWEEPS):
        out = sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R_STAT, seed=LADDER_SEED, sweeps=T, score=score)
        check_ladder(out["draw_state"], "ladder, %d sweeps" % T)
        assert np.all(out["filtered"][:, 4, 0] == 1.0) and np.all(out["filtered"][:, 4, 1:] == 0.0) and np.all(out["filtered"][:, 1, 2] == 0.0)


def test_singletons_are_chromatic_single_site_gibbs():
    rng = np.random.default_rng(1)
    eu, ev, n_used = star_graph()
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 3)
    ptr = np.arange(6)
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    assert colour.tolist() == [0, 1, 1, 1, 0] and n_colours == 2
    want = brute_force(eu, ev, g, d2, n_used, score).astype(np.float64)
    out = sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R_STAT, seed=4, sweeps=12, score=score)
    z = marginal_z(out["draw_state"], want, R_STAT)
    print("star as singletons, 12 sweeps: worst |z| = %.2f" % z)
    assert z <= 5.0 and np.all(out["draw_state"][:, 4] == 0)


# ---- colours ----------------------------------------------------------------------------------------------------------------------------

def test_line_colours():
    ptr = np.array([0, 3, 6, 9])                                               # three parallel lines
    eu, ev = np.array([0, 0, 1, 3, 3, 4, 4, 6, 7]), np.array([1, 3, 2, 4, 6, 5, 7, 7, 8])
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    assert colour.dtype == np.int32 and colour.tolist() == [0, 1, 0] and n_colours == 2
    tie = np.array([0, 3, 6, 9, 11])                                           # a tie line that touches all three
    teu, tev = np.concatenate([eu, [2, 5, 8, 9]]), np.concatenate([ev, [9, 9, 10, 10]])
    colour, n_colours = sections.line_colours(teu, tev, tie)
    assert colour.tolist() == [0, 1, 0, 2] and n_colours == 3
    assert sections.line_colours(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), [0])[1] == 0
    rng = np.random.default_rng(6)
    for _ in range(20):
        L = int(rng.integers(1, 9))
        p = np.concatenate([[0], np.cumsum(rng.integers(0, 4, L))])
        S = int(p[-1])
        m = int(rng.integers(0, 12)) if S > 1 else 0
        a, b = rng.integers(0, max(S, 1), m), rng.integers(0, max(S, 1), m)
        colour, n_colours = sections.line_colours(np.minimum(a, b), np.maximum(a, b), p)
        line = np.searchsorted(p, np.arange(S), side="right") - 1
        for x, y in zip(a, b):
            assert line[x] == line[y] or colour[line[x]] != colour[line[y]]
        assert colour.size == L and (L == 0 or n_colours == colour.max() + 1)


# ---- what a draw depends on ---------------------------------------------------------------------------------------------------------------

def test_determinism_and_continuation():
    eu, ev, g, d2, n_used, score, ptr = ladder_case()
    key = np.array([5, 2 ** 40 + 1, 9, 2 ** 33, 0, 77], dtype=np.int64)
    draw = lambda R, **kw: sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R, **dict(dict(seed=2 ** 40 + 5, sweeps=3, score=score, row_key=key), **kw))      # noqa: E731
    few, many = draw(37), draw(100)
    assert np.array_equal(few["draw_state"], many["draw_state"][:37]) and np.array_equal(few["margin"], many["margin"][:37])
    assert np.array_equal(few["filtered"], many["filtered"][:37])
    assert not np.array_equal(few["draw_state"], draw(37, seed=5)["draw_state"])                      # the seed's high word is used
    assert not np.array_equal(few["draw_state"], draw(37, row_key=key & 0xFFFFFFFF)["draw_state"])    # and a key's
    one = draw(37, sweeps=1)
    on = draw(37, state=one["draw_state"], first_sweep=2)
    assert np.array_equal(on["draw_state"], few["draw_state"]) and np.array_equal(on["filtered"], few["filtered"])
    assert np.array_equal(np.minimum(on["margin"], one["margin"]), few["margin"])
    assert float(sections.philox_uniform(3, 4, 5)) == float(sections.philox_uniform(3, 4, 5, sweep=0)) != float(sections.philox_uniform(3, 4, 5, sweep=1))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_before_the_device(capsys):
    eu, ev, g, d2, n_used, score, ptr = ladder_case()
    d2 = np.nan_to_num(d2)
    ref = lambda eu_=eu, ev_=ev, g_=g, d2_=d2, nu=n_used, ptr_=ptr, R=4, **kw: sections.graph_draw_reference(eu_, ev_, g_, d2_, nu, ptr_, R, **kw)      # noqa: E731
    dev = lambda eu_=eu, ev_=ev, g_=g, d2_=d2, nu=n_used, ptr_=ptr, R=4, **kw: sections.graph_draw(      # noqa: E731
        torch.as_tensor(d2_), g_, eu_, ev_, nu, ptr_, R, **{k: torch.as_tensor(v) if k == "score" else v for k, v in kw.items()})
    for call in (ref, dev):
        with pytest.raises(ValueError, match="not a step"):                   # (0, 2) lies inside the first sequence
            call(eu_=np.array([0, 0, 0, 1, 1, 2, 3, 4]), ev_=np.array([1, 2, 3, 2, 4, 5, 4, 5]), g_=np.ones(8), d2_=np.zeros((8, 3, 3)))
        with pytest.raises(ValueError, match="step 1 -> 2 is missing"):
            call(eu_=np.delete(eu, 2), ev_=np.delete(ev, 2), g_=g[:6], d2_=d2[:6])
        for bad in ([0, 3], [0, 4, 3, 6], [1, 3, 6], [[0, 3, 6]]):
            with pytest.raises(ValueError, match="ptr|decrease"):
                call(ptr_=np.array(bad))
        for kw, match in ((dict(sweeps=-1), "sweeps"), (dict(sweeps=65536), "sweeps"), (dict(sweeps=2.0), "sweeps"), (dict(R=0), "n_draws"), (dict(R=65537), "n_draws"),
                          (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(first_sweep=1), "state"), (dict(sweeps=2, first_sweep=3), "first_sweep"),
                          (dict(state=np.zeros((4, 6), dtype=np.int32)), "state"), (dict(first_sweep=1, state=np.zeros((4, 5), dtype=np.int32)), "state"),
                          (dict(first_sweep=1, state=np.full((4, 6), 2, dtype=np.int32)), "n_used - 1"), (dict(row_key=np.arange(5)), "row_key"),
                          (dict(score=np.zeros((6, 2))), "score"), (dict(nu=np.array([3, 2, 3, 3, 0, 3])), "1 .. n"), (dict(g_=g[:3]), "g must")):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.graph_draw(d2, g, eu, ev, n_used, ptr, 4)
    with pytest.raises(TypeError):
        sections.graph_draw(torch.as_tensor(d2).float(), g, eu, ev, n_used, ptr, 4)
    with pytest.raises(ValueError, match="kernel"):
        sections.graph_draw(torch.as_tensor(d2), g, eu, ev, n_used, ptr, 4, kernel=torch.zeros((7, 3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="block"):
        sections.graph_draw(torch.as_tensor(d2), g, eu, ev, n_used, ptr, 4, block=0)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_graph_draw"):      # host tensors: refused last
        sections.graph_draw(torch.as_tensor(d2), g, eu, ev, n_used, ptr, 4)
    assert len(_lib.SIGNATURES["gbp_section_graph_draw"][1]) == 30
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "geobipy_amd.h")) as f:
        assert "gbp_status gbp_section_graph_draw(" in f.read()

    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--spatial", "300", "--spatial-draws", "16", "--seed", "3", "--draw-sweeps", "5"])
    assert kw["draws"] == 16 and kw["seed"] == 3 and kw["draw_sweeps"] == 5 and kw["max_distance"] == 300.0
    kw = sections.parse_args(["run.npz", "--depth", "150", "--spatial", "300", "--spatial-draws", "16"])[1]
    assert kw["draws"] == 16 and kw["seed"] == 0 and "draw_sweeps" not in kw
    assert "draws" not in sections.parse_args(["run.npz", "--depth", "150", "--spatial", "300"])[1]
    for argv in (["run.npz", "--depth", "10", "--spatial-draws", "4"], ["run.npz", "--depth", "10", "--spatial", "100", "--spatial-draws", "0"],
                 ["run.npz", "--depth", "10", "--spatial", "100", "--draw-sweeps", "3"], ["run.npz", "--depth", "10", "--spatial", "100", "--spatial-draws", "4", "--draw-sweeps", "-1"],
                 ["run.npz", "--depth", "10", "--spatial", "100", "--spatial-draws", "4", "--seed", "-1"]):
        with pytest.raises(SystemExit):
            sections.parse_args(argv)
    capsys.readouterr()


# ---- three planted lines ------------------------------------------------------------------------------------------------------------------

def planted_graph():
    """The planted lines of test_spatial_sections.py as a graph at 1.5 line spacings: (eu, ev, g, d2, n_used, ptr, k, edges, sigma, x, y)."""
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    S, n = k.shape
    rows, n_used = np.tile(np.arange(n, dtype=np.int32), (S, 1)), np.full(S, n)
    eu, ev, g, _ = sections.neighbours(x, y, ptr, n_used, max_distance=1.5 * SPACING)
    d2 = edge_distance_reference(k, edges, sigma, rows, eu, ev, 0.0, Z1_LINES)
    return eu, ev, g, d2, n_used, ptr, k, edges, sigma, x, y


def true_share(draw_state):
    """The share of realisations whose state at the centre of the middle line belongs to the true family (models 10 .. 15)."""
    return float((draw_state[:, S_LINES + S_LINES // 2] >= 10).mean())


def test_the_planted_lines_on_the_rules_alone():
    """Alone the middle line's draws sit on its decoy, the family of the larger share; with its neighbours, on the true family."""
    eu, ev, g, d2, n_used, ptr = planted_graph()[:6]
    R = 512
    alone = true_share(sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R, seed=2, sweeps=0)["draw_state"])
    joint = true_share(sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R, seed=2)["draw_state"])
    print("the true family's share at the centre of the middle line: alone %.3f, across lines after 8 sweeps %.3f" % (alone, joint))
    assert joint > alone
    assert joint > 0.5
