"""Sections across flight lines, the rules alone (geobipy_amd.sections propagate_reference, neighbours): no GPU.

The message passing is held to what it must equal where that is known: the smoothed marginals of ``track_reference`` on a line and
brute-force enumeration on a tree, both within 16 max(e, U), e the fp64 rule's own distance from the rule in long double and
U = 2^-53 (the factor test_sections_gpu.py uses for this arithmetic).  Every case prints used / bound."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, ensembles, sections

U = 2.0 ** -53
LD_ULP = float(np.finfo(np.longdouble).eps)


# ---- the graphs both test files use -------------------------------------------------------------------------------------------------

def line_graph():
    return np.arange(5), np.arange(1, 6), np.array([5, 1, 4, 5, 2, 5])


def star_graph():
    """A star with a tail: 0 in the middle, 1, 2, 3 around it, 4 hangs on 3."""
    return np.array([0, 0, 0, 3]), np.array([1, 2, 3, 4]), np.array([3, 2, 3, 3, 1])


def lattice_graph(rows=3, cols=4):
    """Degree up to 4, and soundings that are the lower endpoint of one edge and the higher endpoint of another."""
    pairs = sorted([(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
                   + [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)])
    return np.array([a for a, _ in pairs]), np.array([b for _, b in pairs]), rows * cols


def graph_inputs(rng, eu, ev, n_used, n):
    """score [S, n], g [E] in [5, 60], d2 [E, n, n] in [0, 0.3] with NaN everywhere outside the prefixes i < m_u, j < m_v."""
    S, E = len(n_used), len(eu)
    score, g, d2 = rng.normal(size=(S, n)), rng.uniform(5.0, 60.0, E), rng.uniform(0.0, 0.3, (E, n, n))
    for e in range(E):
        d2[e, n_used[eu[e]]:, :] = np.nan
        d2[e, :, n_used[ev[e]]:] = np.nan
    return score, g, d2


def brute_force(eu, ev, g, d2, n_used, score, dtype=np.longdouble):
    """The marginals of the graph by enumeration of every configuration."""
    ft = np.dtype(dtype).type
    S, n = len(n_used), d2.shape[1]
    out = np.zeros((S, n), dtype=ft)
    for cfg in itertools.product(*[range(m) for m in n_used]):
        lp = ft(0)
        for s in range(S):
            lp = lp + ft(score[s, cfg[s]])
        for e in range(len(eu)):
            lp = lp - ft(g[e]) * ft(d2[e, cfg[eu[e]], cfg[ev[e]]])
        p = np.exp(lp)
        for s in range(S):
            out[s, cfg[s]] += p
    return out / out.sum(axis=1, keepdims=True)


# ---- the rule where the answer is known ---------------------------------------------------------------------------------------------

def test_a_line_gives_the_smoothed_marginals_of_the_chain():
    rng = np.random.default_rng(0)
    S, n = 6, 5
    eu, ev, n_used = line_graph()
    score, g, d2 = rng.normal(size=(S, n)), rng.uniform(5.0, 60.0, S), rng.uniform(0.0, 0.3, (S, n, n))
    chain = sections.track_reference([0, S], score, g, d2, n_used)["marginal"]
    chain_ld = sections.track_reference([0, S], score, g, d2, n_used, dtype=np.longdouble)["marginal"]
    got = sections.propagate_reference(eu, ev, g[:-1], d2[:-1], n_used, score, sweeps=6)
    got_ld = sections.propagate_reference(eu, ev, g[:-1], d2[:-1], n_used, score, sweeps=6, dtype=np.longdouble)
    e = float(np.abs(got["belief"] - got_ld["belief"]).max())
    bound = 16.0 * max(e, U)
    dist = float(np.abs(got["belief"] - chain).max())
    dist_ld = float(np.abs(got_ld["belief"] - chain_ld).max())
    print("line: e=%.3g used/bound %.3f; long double: %.2f of 16 ulps" % (e, dist / bound, dist_ld / LD_ULP))
    assert got["belief"].dtype == np.float64 and got_ld["belief"].dtype == np.longdouble and got["state"].dtype == np.int32
    assert dist <= bound
    assert dist_ld <= 16.0 * LD_ULP
    assert got["residual"].shape == (6,) and got["residual"][5] == 0.0 and np.all(got["residual"][:3] > 0.0)
    longer = sections.propagate_reference(eu, ev, g[:-1], d2[:-1], n_used, score, sweeps=9)
    assert np.all(longer["residual"][5:] == 0.0) and np.array_equal(longer["residual"][:6], got["residual"])
    assert np.array_equal(longer["belief"], got["belief"])                    # converged: not a bit moves
    for s in range(S):
        assert np.all(got["belief"][s, n_used[s]:] == 0.0) and got["state"][s] == int(np.argmax(got["belief"][s, :n_used[s]]))


def test_a_star_with_a_tail_against_every_configuration():
    rng = np.random.default_rng(1)
    eu, ev, n_used = star_graph()
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 3)
    want = brute_force(eu, ev, g, d2, n_used, score)
    got = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=4)
    got_ld = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=4, dtype=np.longdouble)
    e = float(np.abs(got["belief"] - got_ld["belief"]).max())
    bound = 16.0 * max(e, U)
    dist = float(np.abs(got["belief"] - want).max())
    print("star: e=%.3g used/bound %.3f; long double against the enumeration: %.3g" % (e, dist / bound, float(np.abs(got_ld["belief"] - want).max())))
    assert dist <= bound
    assert float(np.abs(got_ld["belief"] - want).max()) <= 64.0 * LD_ULP
    assert got["residual"][3] == 0.0                                           # the diameter is 3 (1 - 0 - 3 - 4)
    alone = sections.propagate_reference(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((0, 3, 3)), n_used, score, sweeps=2)
    for s in range(5):                                                         # without edges: the normalised w
        w = np.exp(score[s, :n_used[s]])
        assert np.allclose(alone["belief"][s, :n_used[s]], w / w.sum(), rtol=0, atol=4 * U)
    assert np.all(alone["residual"] == 0.0)


def test_loops_converge_and_stay_close_to_the_marginals():
    """A 2 x 3 lattice with 3 states (two loops): the residual dies away and the beliefs stay close to the exact marginals -- the
    distance is the loop approximation DESIGN.md 3.28 records, not an error to fix, so the bar is a loose one."""
    rng = np.random.default_rng(2)
    eu, ev, S = lattice_graph(2, 3)
    n_used = np.full(S, 3)
    _, g, d2 = graph_inputs(rng, eu, ev, n_used, 3)
    got = sections.propagate_reference(eu, ev, g, d2, n_used, None, sweeps=60)
    want = brute_force(eu, ev, g, d2, n_used, np.zeros((S, 3)), dtype=np.float64)
    r = got["residual"]
    print("lattice: residual", r[[0, 4, 9, 19, 59]], "belief - marginal", float(np.abs(got["belief"] - want).max()))
    assert r[59] < 1e-6 and r[59] < r[19] < r[0]
    assert float(np.abs(got["belief"] - want).max()) < 0.1


def test_damping_zero_changes_no_bit():
    rng = np.random.default_rng(3)
    eu, ev, S = lattice_graph()
    n_used = rng.integers(1, 5, S)
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 4)
    plain = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=5)
    zero = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=5, damping=0.0)
    half = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=5, damping=0.5)
    for name in plain:
        assert np.array_equal(plain[name].view(np.int64) if plain[name].dtype == np.float64 else plain[name],
                              zero[name].view(np.int64) if zero[name].dtype == np.float64 else zero[name]), name
    assert not np.array_equal(half["belief"], plain["belief"])
    assert abs(half["residual"][0] - 0.5 * plain["residual"][0]) <= 4 * U      # the first sweep moves half as far


def test_a_zero_total_gives_nan():
    eu, ev, n_used = star_graph()
    score, g, d2 = graph_inputs(np.random.default_rng(4), eu, ev, n_used, 3)
    g[3] = 1e6                                                                 # every entry of the tail's K underflows: its messages are 0 / 0
    d2[3] = np.where(np.isnan(d2[3]), d2[3], 1.0)
    got = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=3)
    assert np.isnan(got["belief"][3, :3]).all() and np.isnan(got["belief"][4, 0]) and np.isnan(got["residual"]).all()
    assert np.isnan(got["belief"][0, :3]).all() and got["state"][0] == 0       # the NaN travels; a NaN never replaces the first state


# ---- the survey graph ---------------------------------------------------------------------------------------------------------------

def test_neighbours_of_three_lines():
    """Lines A (y = 0) and B (y = 100) inside max_distance, C (y = 1000) beyond it; sounding 2 (A, x = 20) has no models; soundings 1
    (A, x = 10) and 4 (B, x = 5) each have two nearest soundings on the other line at exactly the same distance."""
    x = np.array([0.0, 10.0, 20.0, 30.0, 5.0, 15.0, 25.0, 0.0, 10.0, 20.0])
    y = np.array([0.0, 0.0, 0.0, 0.0, 100.0, 100.0, 100.0, 1000.0, 1000.0, 1000.0])
    ptr, n_used = [0, 4, 7, 10], np.array([3, 3, 0, 3, 3, 3, 3, 3, 3, 3])
    assert np.hypot(x[1] - x[4], 100.0) == np.hypot(x[1] - x[5], 100.0) and np.hypot(x[4] - x[0], 100.0) == np.hypot(x[4] - x[1], 100.0)
    eu, ev, g, dist = sections.neighbours(x, y, ptr, n_used, max_distance=150.0)
    assert eu.dtype == np.int32 and ev.dtype == np.int32 and g.dtype == np.float64
    assert list(zip(eu.tolist(), ev.tolist())) == [(0, 1), (0, 4), (1, 4), (1, 5), (3, 6), (4, 5), (5, 6), (7, 8), (8, 9)]
    assert np.all(dist == np.hypot(x[ev] - x[eu], y[ev] - y[eu]))
    assert np.all(g == 100.0 / (2.0 * 0.1 * 0.1 * np.maximum(dist, 1.0)))      # the formula of ``steps``
    along = ev == eu + 1
    assert np.all(g[along] == sections.steps(x, y, ptr=ptr)[eu[along]])        # and its numbers where both apply
    partner = sections.partners(ptr, n_used)
    assert sorted(zip(eu[along].tolist(), ev[along].tolist())) == [(s, int(q)) for s, q in enumerate(partner) if q >= 0]
    other = sections.neighbours(x, y, ptr, n_used, max_distance=150.0, tau=0.2, length=50.0, min_distance=20.0)
    assert np.all(other[2] == 50.0 / (2.0 * 0.2 * 0.2 * np.maximum(dist, 20.0)))
    near = sections.neighbours(x, y, ptr, n_used, max_distance=99.0)            # below the line spacing: the lines alone
    assert list(zip(near[0].tolist(), near[1].tolist())) == [(0, 1), (4, 5), (5, 6), (7, 8), (8, 9)]
    far = sections.neighbours(x, y, ptr, None, max_distance=1000.0)             # everything has models, and C comes within reach
    assert (2, 5) in list(zip(far[0].tolist(), far[1].tolist())) and (4, 7) in list(zip(far[0].tolist(), far[1].tolist()))
    assert np.all(np.diff(far[0].astype(np.int64) * 10 + far[1]) > 0)
    with pytest.raises(TypeError):
        sections.neighbours(x, y, ptr, n_used)                                  # max_distance is not guessed
    for kw in (dict(max_distance=0.0), dict(max_distance=np.inf), dict(max_distance=150.0, tau=0.0)):
        with pytest.raises(ValueError):
            sections.neighbours(x, y, ptr, n_used, **kw)
    in_ptr, in_edge = sections.incoming(eu, ev, 10)
    assert in_ptr.tolist() == [0, 2, 5, 5, 6, 9, 12, 14, 15, 17, 18] and in_edge[:5].tolist() == [1, 3, 0, 5, 7]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_library():
    d2, g, n_used = torch.zeros((3, 4, 4), dtype=torch.float64), np.ones(3), np.array([4, 1, 2, 4])
    eu, ev = np.array([0, 0, 2]), np.array([1, 3, 3])
    for call in (lambda eu_, ev_, g_=g, d2_=d2, nu=n_used, **kw: sections.propagate(d2_, g_, eu_, ev_, nu, len(nu), **kw),
                 lambda eu_, ev_, g_=g, d2_=d2, nu=n_used, **kw: sections.propagate_reference(eu_, ev_, g_, d2_, nu, **kw)):
        for bad, match in ((([0, 2, 0], [3, 3, 1]), "sorted"), (([0, 0, 0], [1, 1, 3]), "duplicates"), (([0, 3, 2], [1, 3, 3]), "eu < ev"),
                           (([0, 2, 2], [1, 1, 3]), "eu < ev"), (([0, 0, 2], [1, 3, 4]), "eu < ev"), (([0, 0], [1, 3]), "one integer per edge")):
            with pytest.raises(ValueError, match=match):
                call(np.array(bad[0]), np.array(bad[1]))
        with pytest.raises(ValueError, match="damping"):
            call(eu, ev, damping=1.0)
        with pytest.raises(ValueError, match="damping"):
            call(eu, ev, damping=-0.1)
        with pytest.raises(ValueError, match="sweeps"):
            call(eu, ev, sweeps=0)
        with pytest.raises(ValueError, match="n <= 256"):
            call(eu[:0], ev[:0], g_=g[:0], d2_=torch.zeros((1, 257, 257), dtype=torch.float64)[:0])
        with pytest.raises(ValueError, match="1 .. n"):
            call(eu, ev, nu=np.array([4, 0, 2, 4]))
        with pytest.raises(ValueError, match="g must"):
            call(eu, ev, g_=g[:2])
        with pytest.raises(ValueError, match="score"):
            call(eu, ev, score=torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.propagate(d2.numpy(), g, eu, ev, n_used, 4)
    with pytest.raises(ValueError, match="n_used"):
        sections.propagate(d2, g, eu, ev, n_used, 5)
    with pytest.raises(TypeError):
        sections.propagate(d2.float(), g, eu, ev, n_used, 4)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_propagate"):
        sections.propagate(d2, g, eu, ev, n_used, 4)

    S, ns, K = 4, 8, 4
    k = torch.ones((S, ns), dtype=torch.int32)
    ens = ensembles.Ensemble(k, torch.full((S, ns, K), float("inf"), dtype=torch.float64), torch.ones((S, ns, K), dtype=torch.float64),
                             torch.zeros((S, ns), dtype=torch.float64), (k > 0).sum(dim=1), 1, torch.zeros(S, dtype=torch.float64))
    x, y = np.array([0.0, 10.0, 0.0, 10.0]), np.array([0.0, 0.0, 50.0, 50.0])
    with pytest.raises(TypeError):
        sections.spatial(ens, x, y, 10.0, ptr=[0, 2, 4])
    for kw in (dict(max_models=257), dict(max_models=0), dict(sweeps=0), dict(damping=1.0), dict(tau=0.0), dict(max_distance=-1.0), dict(ptr=[0, 1]),
               dict(budget_bytes=0), dict(measure="log"), dict(score=torch.zeros((4, 5), dtype=torch.float64))):
        with pytest.raises(ValueError):
            sections.spatial(ens, x, y, 10.0, **dict(dict(ptr=[0, 2, 4], max_distance=60.0), **kw))
    with pytest.raises(ValueError, match="max_models or max_distance.*budget_bytes"):      # 4 edges x 8 x 8 doubles do not fit 2 000 bytes
        sections.spatial(ens, x, y, 10.0, ptr=[0, 2, 4], max_distance=60.0, budget_bytes=2000)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.spatial(ens, x, y, 10.0, ptr=[0, 2, 4], max_distance=60.0)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.edge_distance(ens, torch.zeros((S, 8), dtype=torch.int32).numpy(), [0], [1], 0.0, 10.0)
    with pytest.raises(ValueError, match="sorted"):
        sections.edge_distance(ens, torch.zeros((S, 8), dtype=torch.int32), [1, 0], [2, 1], 0.0, 10.0)
    survey = dict(ensemble_k=k.numpy(), ensemble_edges=ens.edges.numpy(), ensemble_sigma=ens.sigma.numpy(), line=np.zeros(4), x=x, y=y)
    with pytest.raises(ValueError, match="max_distance"):
        sections.from_survey(survey, 10.0, spatial=dict(sweeps=3))
    with pytest.raises(ValueError, match="max_distance"):
        sections.spatial_from_survey(survey, 10.0)
    with pytest.raises(ValueError, match="ptr is not taken"):
        sections.spatial_from_survey(survey, 10.0, max_distance=60.0, ptr=[0, 4])


def test_the_command_line_takes_spatial(capsys):
    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--spatial", "300", "--sweeps", "12", "--damping", "0.25", "--max-models", "32"])
    assert path == "run.npz" and kw == dict(z1=150.0, z0=0.0, measure="linear", tau=0.1, length=100.0, max_models=32, chains=1, device="cuda:0",
                                            max_distance=300.0, sweeps=12, damping=0.25)
    assert sections.output_path("a/run.npz", sections.SPATIAL_SUFFIX) == "a/run.spatial.npz"
    assert "max_distance" not in sections.parse_args(["run.npz", "--depth", "150"])[1]
    for argv in (["run.npz", "--depth", "10", "--spatial", "0"], ["run.npz", "--depth", "10", "--sweeps", "3"], ["run.npz", "--depth", "10", "--damping", "0.1"],
                 ["run.npz", "--depth", "10", "--spatial", "100", "--damping", "1"], ["run.npz", "--depth", "10", "--spatial", "100", "--sweeps", "0"],
                 ["run.npz", "--depth", "10", "--spatial", "100", "--max-models", "300"], ["run.npz", "--depth", "10", "--spatial", "100", "--draws", "4"],
                 ["run.npz", "--depth", "10", "--spatial", "100", "--no-marginals"]):
        with pytest.raises(SystemExit):
            sections.parse_args(argv)
    capsys.readouterr()


def test_the_signature_declares_the_entry():
    assert len(_lib.SIGNATURES["gbp_section_propagate"][1]) == 21
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "geobipy_amd.h")) as f:
        assert "gbp_status gbp_section_propagate(" in f.read()


# ---- three planted lines ------------------------------------------------------------------------------------------------------------

S_LINES, N_LINES, Z1_LINES, SPACING, DECOY = 8, 16, 120.0, 100.0, 50.0


def planted_lines():
    """Three parallel lines 100 m apart of 8 soundings 25 m apart, 16 three-layer models each (K = 4), built as the planted line of
    test_sections.py is: the first interface of the true family lies at 30 + 10 sin(s / 6) m, +- 1 m of normal jitter, under all three
    lines.  The outer lines are unambiguous.  On the middle line 10 of the 16 models of EVERY sounding belong to a decoy family whose
    first interface is flat at 50 m, 11 to 20 m below the true one, with a third of the jitter in every parameter: the larger share
    and the smoother path, so alone the line has no reason to leave it.  Returns (k [S, n], edges,
    sigma [S, n, K], x, y, ptr, truth [S]) with the soundings of line l in rows 8 l .. 8 l + 7."""
    rng = np.random.default_rng(11)
    L, Sl, n, K = 3, S_LINES, N_LINES, 4
    S = L * Sl
    truth = np.tile(30.0 + 10.0 * np.sin(np.arange(Sl) / 6.0), L)
    k = np.full((S, n), 3, dtype=np.int32)
    edges, sigma = np.full((S, n, K), np.inf), np.full((S, n, K), np.nan)
    for s in range(S):
        top = truth[s] + rng.normal(0.0, 1.0, n)
        if s // Sl == 1:
            top[:10] = DECOY + rng.normal(0.0, 1.0 / 3.0, 10)
        tight = np.where((np.arange(n) < 10) & (s // Sl == 1), 1.0 / 3.0, 1.0)
        edges[s, :, 0] = top
        edges[s, :, 1] = 80.0 + tight * rng.normal(0.0, 1.0, n)
        sigma[s, :, :3] = 10.0 ** (np.array([-2.0, -0.5, -1.5]) + tight[:, None] * rng.normal(0.0, 0.05, (n, 3)))
    x, y = np.tile(25.0 * np.arange(Sl), L), np.repeat(SPACING * np.arange(L), Sl)
    return k, edges, sigma, x, y, np.arange(L + 1) * Sl, truth


def edge_distance_reference(k, edges, sigma, rows, eu, ev, z0, z1):
    """d2 [E, n, n] through ``cross_distance_reference``, one edge at a time."""
    out = np.zeros((len(eu), rows.shape[1], rows.shape[1]))
    for e in range(len(eu)):
        partner = np.full(k.shape[0], -1)
        partner[eu[e]] = ev[e]
        pair = [eu[e], ev[e]]
        out[e] = sections.cross_distance_reference(k[pair], edges[pair], sigma[pair], rows[pair], np.array([1, -1]), z0, z1)[0]
    return out


def test_the_planted_lines_on_the_rules_alone():
    """What coupling across lines is for: alone, the middle line sits on its decoy; with its neighbours, on the true family."""
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    S, n = k.shape
    rows, n_used = np.tile(np.arange(n, dtype=np.int32), (S, 1)), np.full(S, n)
    middle = np.arange(S_LINES, 2 * S_LINES)
    beliefs = {}
    for reach in (0.5 * SPACING, 1.5 * SPACING):
        eu, ev, g, dist = sections.neighbours(x, y, ptr, n_used, max_distance=reach)
        assert eu.size == (21 if reach < SPACING else 21 + 16) and (reach < SPACING or np.all(dist[ev != eu + 1] == SPACING))
        d2 = edge_distance_reference(k, edges, sigma, rows, eu, ev, 0.0, Z1_LINES)
        beliefs[reach] = sections.propagate_reference(eu, ev, g, d2, n_used, None, sweeps=8)
    alone, joint = beliefs[0.5 * SPACING], beliefs[1.5 * SPACING]
    assert np.all(alone["residual"][7:] == 0.0)                               # three trees of diameter 7
    decoy_alone, decoy_joint = alone["belief"][middle, :10].sum(axis=1), joint["belief"][middle, :10].sum(axis=1)
    print("the decoy's share of the middle line: alone %.3f .. %.3f, with its neighbours at most %.3g; residual %.3g"
          % (decoy_alone.min(), decoy_alone.max(), decoy_joint.max(), joint["residual"][-1]))
    assert np.all(alone["state"][middle] < 10) and np.all(decoy_alone > 0.625)
    assert np.all(joint["state"][middle] >= 10) and np.all(decoy_joint < 1e-3)
    chosen = edges[np.arange(S), joint["state"], 0]
    assert np.all(np.abs(chosen - truth) <= 4.0)
    partner = sections.partners(ptr, n_used)                                   # and the most probable path of the line alone, as sections() picks it
    chain = sections.cross_distance_reference(k, edges, sigma, rows, partner, 0.0, Z1_LINES)
    path = sections.track_reference(ptr, None, sections.steps(x, y, ptr=ptr), chain, n_used, marginals=False)["state"]
    assert np.all(path[middle] < 10) and np.all(np.abs(edges[middle, path[middle], 0] - DECOY) <= 2.0)
