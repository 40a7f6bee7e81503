"""Sections across flight lines on the device (csrc/gbp_section_graph.h k_graph_kernel / k_graph_init / k_graph_sweep /
k_graph_residual / k_graph_belief through gbp_section_propagate; geobipy_amd.sections propagate, edge_distance, spatial).

The device is held to ``sections.propagate_reference`` in fp64: belief and residual within 16 max(e, U), e the fp64 rule's own distance
from the rule in long double, measured per case, and U = 2^-53; NaN where the rule has NaN; ``state`` the first maximum of the device's
own belief.  Every case prints used / bound."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, sections
from test_families_gpu import _to_device
from test_spatial_sections import DECOY, S_LINES, SPACING, U, Z1_LINES, graph_inputs, lattice_graph, line_graph, planted_lines, star_graph


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _device(eu, ev, g, d2, n_used, score, **kw):
    dev = _dev()
    out = sections.propagate(torch.as_tensor(d2).to(dev), g, eu, ev, n_used, len(n_used), score=None if score is None else torch.as_tensor(score).to(dev), **kw)
    torch.cuda.synchronize()
    return out


def _first_max(b, m):
    return sections.first_max(b[:m])


GRAPHS = ("line", "star", "lattice", "isolated")


def _graph(name, n, rng):
    """eu, ev and a ragged n_used that holds 1 and n."""
    if name == "line":
        eu, ev, nu = line_graph()
        S = nu.size
    elif name == "star":
        eu, ev, nu = star_graph()
        S = nu.size
    elif name == "lattice":
        eu, ev, S = lattice_graph()
    else:                                                                      # sounding 2 has no edge; 5 neither, at the end
        eu, ev, S = np.array([0, 0, 1, 3]), np.array([1, 3, 4, 4]), 6
    n_used = rng.integers(1, n + 1, S)
    n_used[0], n_used[S - 2] = n, 1
    return eu, ev, n_used


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("name", GRAPHS)
def test_propagate_against_the_rule(name, n):
    rng = np.random.default_rng(1000 * GRAPHS.index(name) + n)
    eu, ev, n_used = _graph(name, n, rng)
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, n)
    S = n_used.size
    for sweeps in (1, 2, 7):
        for lam in (0.0, 0.5):
            got = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=sweeps, damping=lam))
            ref = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=sweeps, damping=lam)
            ld = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=sweeps, damping=lam, dtype=np.longdouble)
            assert got["belief"].shape == (S, n) and got["belief"].dtype == np.float64 and got["state"].dtype == np.int32 and got["residual"].shape == (sweeps,)
            assert np.all(np.isfinite(ref["belief"])) and np.all(np.isfinite(ref["residual"]))      # the inputs stay clear of underflow
            assert np.array_equal(np.isnan(got["belief"]), np.isnan(ref["belief"])) and np.array_equal(np.isnan(got["residual"]), np.isnan(ref["residual"]))
            e_b, e_r = float(np.abs(ref["belief"] - ld["belief"]).max()), float(np.abs(ref["residual"] - ld["residual"]).max())
            b_b, b_r = 16.0 * max(e_b, U), 16.0 * max(e_r, U)
            d_b, d_r = float(np.abs(got["belief"] - ref["belief"]).max()), float(np.abs(got["residual"] - ref["residual"]).max())
            print("%s n=%d sweeps=%d damping=%.1f: belief e=%.3g used/bound %.3f; residual e=%.3g used/bound %.3f"
                  % (name, n, sweeps, lam, e_b, d_b / b_b, e_r, d_r / b_r))
            assert d_b <= b_b
            assert d_r <= b_r
            for s in range(S):
                assert np.all(got["belief"][s, n_used[s]:] == 0.0) and got["state"][s] == _first_max(got["belief"][s], n_used[s])
            assert float(np.abs(got["belief"].sum(axis=1) - 1.0).max()) <= b_b + 4 * U * n
    if name == "isolated":                                                     # no edges: the normalised w
        for s in (2, 5):
            w = np.exp(score[s, :n_used[s]])
            assert float(np.abs(got["belief"][s, :n_used[s]] - w / w.sum()).max()) <= 16.0 * U


def test_nan_where_the_rule_has_nan():
    eu, ev, n_used = star_graph()
    score, g, d2 = graph_inputs(np.random.default_rng(4), eu, ev, n_used, 3)
    g[3] = 1e6                                                                 # the tail's K underflows: its messages are 0 / 0
    d2[3] = np.where(np.isnan(d2[3]), d2[3], 1.0)
    for sweeps in (1, 3):
        got = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=sweeps))
        ref = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=sweeps)
        assert np.isnan(ref["belief"]).any() and np.isnan(ref["residual"]).all()
        assert np.array_equal(np.isnan(got["belief"]), np.isnan(ref["belief"])) and np.array_equal(np.isnan(got["residual"]), np.isnan(ref["residual"]))
        ok = ~np.isnan(ref["belief"])
        assert float(np.abs(got["belief"][ok] - ref["belief"][ok]).max(initial=0.0)) <= 16.0 * U * 4
        assert np.array_equal(got["state"], ref["state"])                      # a NaN never replaces the first state


def test_a_call_repeats_its_own_bits():
    rng = np.random.default_rng(77)
    eu, ev, n_used = _graph("lattice", 130, rng)
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 130)
    for lam in (0.0, 0.5):
        a, b = _device(eu, ev, g, d2, n_used, score, sweeps=5, damping=lam), _device(eu, ev, g, d2, n_used, score, sweeps=5, damping=lam)
        for name in ("belief", "state", "residual"):
            assert torch.equal(_bits(a[name]), _bits(b[name])), (lam, name)
    zero = _device(eu, ev, g, d2, n_used, score, sweeps=5)
    assert torch.equal(_bits(zero["belief"]), _bits(_device(eu, ev, g, d2, n_used, score, sweeps=5, damping=0.0)["belief"]))
    flat = _device(eu, ev, g, d2, n_used, None, sweeps=5)                      # score None: zeros
    zeros = _device(eu, ev, g, d2, n_used, np.zeros((n_used.size, 130)), sweeps=5)
    assert torch.equal(_bits(flat["belief"]), _bits(zeros["belief"]))


@pytest.mark.parametrize("name,diameter", [("line", 5), ("star", 3)])
def test_a_tree_converges_in_its_diameter(name, diameter):
    rng = np.random.default_rng(5 + diameter)
    eu, ev, n_used = _graph(name, 65, rng)
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, 65)
    got = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=diameter + 3))
    print(name, "residual", got["residual"])
    assert np.all(got["residual"][diameter:] == 0.0) and np.all(got["residual"][:2] > 0.0)
    again = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=diameter))
    assert np.array_equal(again["belief"], got["belief"])                      # converged: not a bit moves


def _planted():
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    return _to_device(k, edges, sigma), edges, x, y, ptr, truth


def test_edge_distance_is_the_cross_distance_kernel():
    ens, _, x, y, ptr, _ = _planted()
    S, n = ens.k.shape
    rows = torch.arange(n, dtype=torch.int32, device=_dev())[None, :].repeat(S, 1)
    rows[3, 5:] = -1                                                           # a sounding with fewer models
    eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * SPACING)
    assert eu.size == 37 and np.bincount(eu).max() == 2                        # two passes
    for measure, z0 in (("linear", 0.0), ("log", 2.0)):
        got = sections.edge_distance(ens, rows, eu, ev, z0, Z1_LINES, measure=measure)
        assert got.shape == (37, n, n) and got.dtype == torch.float64
        for e in range(eu.size):
            partner = np.full(S, -1, dtype=np.int32)
            partner[eu[e]] = ev[e]
            want = sections.cross_distance(ens, rows, partner, z0, Z1_LINES, measure=measure)[int(eu[e])]
            assert torch.equal(_bits(got[e]), _bits(want)), (measure, e)
    assert bool(torch.isnan(got[np.flatnonzero(eu == 3)[0], 5:]).all())
    none = sections.edge_distance(ens, rows, eu[:0], ev[:0], 0.0, Z1_LINES)
    assert none.shape == (0, n, n)


def test_the_planted_lines_on_the_device():
    ens, edges, x, y, ptr, truth = _planted()
    S, n = ens.k.shape
    middle = np.arange(S_LINES, 2 * S_LINES)
    depth_edges = np.arange(0.0, Z1_LINES + 1.0, 2.5)
    products = dict(depth_edges=depth_edges, percentiles=(50,))
    lines = _numpy(sections.sections(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, products=products))
    # (a) no edge across lines: three trees, the smoothed marginals of the chains
    alone = _numpy(sections.spatial(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, max_distance=0.5 * SPACING, sweeps=8, products=products))
    assert alone["edge_u"].size == 21 and np.all(alone["edge_v"] == alone["edge_u"] + 1) and alone["residual"][7] == 0.0
    partner = sections.partners(ptr, lines["n_used"])
    d2 = sections.cross_distance(ens, torch.as_tensor(lines["rows"]).to(_dev()), partner, 0.0, Z1_LINES).cpu().numpy()
    g = sections.steps(x, y, ptr=ptr)
    ref = sections.track_reference(ptr, None, g, d2, lines["n_used"])["marginal"]
    ld = sections.track_reference(ptr, None, g, d2, lines["n_used"], dtype=np.longdouble)["marginal"]
    e = float(np.abs(ref - ld).max())
    bound = 16.0 * max(e, U)
    dist = float(np.abs(alone["weight"] - lines["weight"]).max())
    print("three lines alone: e=%.3g used/bound %.3f" % (e, dist / bound))
    assert dist <= bound
    assert np.all(np.abs(edges[middle, lines["state"][middle], 0] - DECOY) <= 2.0)      # the line alone sits on its decoy
    assert np.all(alone["state"][middle] < 10)
    # (b) 1.5 line spacings: the neighbours decide
    joint = _numpy(sections.spatial(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, max_distance=1.5 * SPACING, products=products))
    assert joint["edge_u"].size == 37 and joint["residual"].shape == (32,) and joint["residual"][-1] < 1e-6
    assert np.all(joint["state"][middle] >= 10) and np.all(np.abs(edges[np.arange(S), joint["state"], 0] - truth) <= 4.0)
    assert np.all(joint["weight"][middle, :10].sum(axis=1) < 1e-3) and np.all(joint["n_effective"] >= 1.0 - 1e-12) and np.all(joint["n_effective"] <= n + 1e-9)
    assert np.array_equal(joint["slot"], joint["state"]) and np.array_equal(joint["section_edges"], edges[np.arange(S), joint["state"]])
    eu, ev, g2, length = sections.neighbours(x, y, ptr, None, max_distance=1.5 * SPACING)
    assert np.array_equal(joint["edge_u"], eu) and np.array_equal(joint["edge_v"], ev) and np.array_equal(joint["edge_length"], length)
    assert np.all(joint["edge_distance"] < 0.45) and np.all(joint["edge_distance"] >= 0.0)      # no jump between families on any edge
    # the median follows: between the true interface and the decoy the true family is in its conductive layer, the decoy is not
    for s in middle:
        cell = int(np.ceil((truth[s] + 3.0) / 2.5))                           # the first cell 3 m (3 sigma of the jitter) or more below the true interface
        assert depth_edges[cell] >= truth[s] + 3.0 and depth_edges[cell + 1] <= DECOY - 2.0
        assert lines["lateral_percentile_50"][s, cell] < -1.5 and alone["lateral_percentile_50"][s, cell] < -1.5
        assert joint["lateral_percentile_50"][s, cell] > -1.0
    # the rule on the device's own distances
    rows = torch.as_tensor(joint["rows"]).to(_dev())
    d2e = sections.edge_distance(ens, rows, eu, ev, 0.0, Z1_LINES).cpu().numpy()
    rule = sections.propagate_reference(eu, ev, g2, d2e, joint["n_used"], None, sweeps=32)
    assert np.allclose(joint["weight"], rule["belief"], rtol=0, atol=1e-13) and np.array_equal(joint["state"], rule["state"])
    # a sounding without models is left out of the graph
    kk = ens.k.clone()
    kk[9] = 0
    cut = _numpy(sections.spatial(ens._replace(k=kk), x, y, Z1_LINES, ptr=ptr, max_models=n, max_distance=1.5 * SPACING))
    assert cut["state"][9] == -1 and cut["slot"][9] == -1 and np.isnan(cut["weight"][9]).all() and np.isnan(cut["n_effective"][9]) and cut["section_k"][9] == 0
    assert not np.any((cut["edge_u"] == 9) | (cut["edge_v"] == 9)) and np.all(cut["state"][np.arange(S) != 9] >= 0)
    assert np.all(cut["state"][middle[2:]] >= 10)


def test_from_survey_and_the_command_line(tmp_path):
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    survey = dict(ensemble_k=k, ensemble_edges=edges, ensemble_sigma=sigma, line=np.repeat([10, 20, 30], S_LINES), x=x, y=y, fiducial=np.arange(k.shape[0]))
    direct = _numpy(sections.spatial_from_survey(survey, Z1_LINES, max_models=16, max_distance=150.0, sweeps=12))
    both = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, spatial=dict(max_models=16, max_distance=150.0, sweeps=12)))
    plain = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16))
    assert {"weight", "state", "edge_u", "residual", "line", "fiducial", "x", "y"} <= set(direct) and direct["residual"].shape == (12,)
    for name in direct:
        if name not in ("line", "fiducial", "x", "y"):
            assert np.array_equal(both["spatial_" + name], direct[name], equal_nan=True), name
    assert set(plain) == {name for name in both if not name.startswith("spatial_")}
    assert all(np.array_equal(both[name], plain[name], equal_nan=True) for name in plain)
    path = str(tmp_path / "survey.npz")
    np.savez(path, **survey)
    written = sections.main([path, "--depth", "120", "--spatial", "150", "--sweeps", "12", "--max-models", "16"])
    assert written == str(tmp_path / "survey.spatial.npz")
    f = sections.load(written)
    assert set(f) == set(direct) and all(np.array_equal(f[name], direct[name], equal_nan=True) for name in direct)


def test_the_c_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    S, E, n, sweeps = 3, 2, 4, 2
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)      # noqa: E731
    eu, ev, nu, in_ptr, in_edge = i32([0, 1]), i32([1, 2]), i32([4, 4, 4]), i32([0, 1, 3, 4]), i32([1, 0, 3, 2])
    score, g, d2, K, w, mu, resid, belief, residual = f64(S, n), f64(E), f64(E, n, n), f64(E, n, n), f64(S, n), f64(2, 2 * E, n), f64(sweeps, 2 * E), f64(S, n), f64(sweeps)
    state = torch.full((S,), 7, dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else a.data_ptr()                          # noqa: E731
    call = lambda S_=S, E_=E, n_=n, eu_=eu, ev_=ev, nu_=nu, score_=score, g_=g, d2_=d2, ptr_=in_ptr, edge_=in_edge, sweeps_=sweeps, lam=0.0, K_=K, w_=w, mu_=mu, \
        resid_=resid, belief_=belief, state_=state, residual_=residual: \
        lib.gbp_section_propagate(S_, E_, n_, p(eu_), p(ev_), p(nu_), p(score_), p(g_), p(d2_), p(ptr_), p(edge_), sweeps_, lam, p(K_), p(w_), p(mu_), p(resid_),
                                  p(belief_), p(state_), p(residual_), st)     # noqa: E731
    for kw in (dict(S_=-1), dict(E_=-1), dict(E_=2 ** 30), dict(n_=0), dict(n_=257), dict(sweeps_=0), dict(lam=1.0), dict(lam=-0.5), dict(lam=float("nan")),
               dict(S_=1), dict(S_=2 ** 31 - 1, E_=2 ** 29), dict(eu_=None), dict(ev_=None), dict(nu_=None), dict(score_=None), dict(g_=None), dict(d2_=None),
               dict(ptr_=None), dict(edge_=None), dict(K_=None), dict(w_=None), dict(mu_=None), dict(resid_=None), dict(belief_=None), dict(state_=None),
               dict(residual_=None)):
        assert call(**kw) != 0 and b"gbp_section_propagate" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    for t in (K, w, mu, resid, belief, residual):
        assert bool((t == 7.0).all())                                          # nothing was written
    assert bool((state == 7).all())
    none = sections.propagate(torch.zeros((0, 4, 4), dtype=torch.float64, device=dev), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                              np.zeros(0, dtype=np.int32), 0, sweeps=3)
    assert none["belief"].shape == (0, 4) and none["state"].shape == (0,) and bool((none["residual"] == 0.0).all())
    score = torch.tensor([[0.5, -1.0, 9.0, 9.0], [0.0, 1.0, 2.0, 3.0]], dtype=torch.float64, device=dev)
    apart = sections.propagate(torch.zeros((0, 4, 4), dtype=torch.float64, device=dev), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                               np.array([2, 4]), 2, score=score, sweeps=3)      # soundings without a single edge: the normalised w, nothing to sweep
    w = np.exp(score.cpu().numpy()) * np.array([[1, 1, 0, 0], [1, 1, 1, 1]])
    assert float(np.abs(apart["belief"].cpu().numpy() - w / w.sum(axis=1, keepdims=True)).max()) <= 16.0 * U
    assert apart["state"].tolist() == [0, 3] and bool((apart["residual"] == 0.0).all())
