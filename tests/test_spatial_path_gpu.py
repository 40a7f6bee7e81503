"""The most probable section across flight lines on the device (csrc/gbp_section_graph_path.h k_graph_maxsum / k_graph_maxmarginal /
k_graph_condition through gbp_section_graph_path and gbp_section_graph_refine; geobipy_amd.sections graph_path, refine, spatial(path=);
DESIGN.md 3.32).

The device is held to ``sections.graph_path_reference`` with ``==`` and no tolerance: the rule has no exp and no sum whose order could
differ, so max_marginal, residual, decoded_state, refine_moves, candidate_state and state must agree entry for entry (NaN where the
rule has NaN).  ``log_score`` is ``graph_log_score`` on both sides, a sum torch orders differently on the two devices: it is compared
within 64 ulp of the largest partial sum.  Outside the prefixes d2 holds -inf: a candidate read from there would be +inf and win."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, sections
from test_families_gpu import _to_device
from test_spatial_sections import S_LINES, SPACING, U, Z1_LINES, graph_inputs, lattice_graph, line_graph, planted_lines, star_graph

EXACT = ("max_marginal", "residual", "decoded_state", "refine_moves", "candidate_state", "state")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _device(eu, ev, g, d2, n_used, score, **kw):
    dev = _dev()
    out = sections.graph_path(torch.as_tensor(d2).to(dev), g, eu, ev, n_used, len(n_used), score=None if score is None else torch.as_tensor(score).to(dev), **kw)
    torch.cuda.synchronize()
    return out


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


def _inputs(rng, eu, ev, n_used, n):
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, n)
    return score, g, np.where(np.isnan(d2), -np.inf, d2)


def _same(got, ref, what):
    for name in EXACT:
        assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype, (what, name, got[name].shape, got[name].dtype)
        assert np.array_equal(got[name], ref[name], equal_nan=got[name].dtype == np.float64), (what, name)
    assert int(got["chosen"]) == int(ref["chosen"]), what
    scale = max(1.0, float(np.abs(ref["candidate_log_score"][np.isfinite(ref["candidate_log_score"])]).max(initial=0.0)))
    ok = np.isfinite(ref["candidate_log_score"])
    assert np.array_equal(np.isfinite(got["candidate_log_score"]), ok), what
    assert float(np.abs(got["candidate_log_score"][ok] - ref["candidate_log_score"][ok]).max(initial=0.0)) <= 64.0 * 2.0 * U * scale * len(ref["state"]), what
    assert got["log_score"] == got["candidate_log_score"][int(got["chosen"])], what


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("name", GRAPHS)
def test_graph_path_against_the_rule(name, n):
    rng = np.random.default_rng(1000 * GRAPHS.index(name) + n)
    eu, ev, n_used = _graph(name, n, rng)
    score, g, d2 = _inputs(rng, eu, ev, n_used, n)
    S = n_used.size
    given = rng.integers(0, n_used[None, :], (2, S))
    moved = 0
    for sweeps in (1, 5):
        for lam in (0.0, 0.5):
            got = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=sweeps, damping=lam, refine=6, candidates=given))
            ref = sections.graph_path_reference(eu, ev, g, d2, n_used, score, sweeps=sweeps, damping=lam, refine=6, candidates=given)
            assert np.all(np.isfinite(ref["residual"])) and got["residual"].shape == (sweeps,) and got["refine_moves"].shape == (3, 6)
            _same(got, ref, (name, n, sweeps, lam))
            for s in range(S):
                assert np.all(got["max_marginal"][s, n_used[s]:] == -np.inf) and got["max_marginal"][s, :n_used[s]].max() == 0.0
            moved += int(ref["refine_moves"].sum())
    print("%s n=%d: %d refine moves over the four calls" % (name, n, moved))
    assert n == 1 or moved > 0                                                 # the random candidates are not modes: the ascent was exercised
    alone = _numpy(_device(eu[:0], ev[:0], g[:0], d2[:0], n_used, score, sweeps=2))      # no edges: every sounding's best model
    assert np.all(alone["residual"] == 0.0) and alone["state"].tolist() == [sections._first_above(score[s, :n_used[s]])[0] for s in range(S)]


def test_minus_infinity_and_nan_where_the_rule_has_them():
    rng = np.random.default_rng(9)
    eu, ev, n_used = star_graph()
    score, g, d2 = _inputs(rng, eu, ev, n_used, 3)
    barred = score.copy()
    barred[0, 1], barred[3, 0], barred[4, 0] = -np.inf, -np.inf, 0.5          # models ruled out, never all of a sounding
    for sweeps in (1, 4):
        got = _numpy(_device(eu, ev, g, d2, n_used, barred, sweeps=sweeps, candidates=np.array([[0, 0, 0, 1, 0]])))
        ref = sections.graph_path_reference(eu, ev, g, d2, n_used, barred, sweeps=sweeps, candidates=np.array([[0, 0, 0, 1, 0]]))
        assert np.all(np.isfinite(ref["residual"])) and ref["max_marginal"][0, 1] == -np.inf and ref["state"][0] != 1 and ref["state"][3] != 0
        _same(got, ref, ("-inf", sweeps))
    lost = score.copy()
    lost[4, :] = np.nan                                                        # every candidate of the message 4 -> 3 is NaN: it is NaN, and it travels
    for sweeps in (1, 4):
        got = _numpy(_device(eu, ev, g, d2, n_used, lost, sweeps=sweeps, candidates=np.array([[0, 0, 0, 1, 0]])))
        ref = sections.graph_path_reference(eu, ev, g, d2, n_used, lost, sweeps=sweeps, candidates=np.array([[0, 0, 0, 1, 0]]))
        assert np.isnan(ref["residual"]).all() and np.isnan(ref["max_marginal"][3, :3]).all() and np.isnan(ref["max_marginal"][4, 0])
        assert np.isnan(ref["candidate_log_score"]).all()
        for name in EXACT:
            assert np.array_equal(got[name], ref[name], equal_nan=got[name].dtype == np.float64), (sweeps, name)
        assert np.isnan(got["candidate_log_score"]).all() and int(got["chosen"]) == int(ref["chosen"]) == 0


def test_a_call_repeats_its_own_bits():
    rng = np.random.default_rng(77)
    eu, ev, n_used = _graph("lattice", 130, rng)
    score, g, d2 = _inputs(rng, eu, ev, n_used, 130)
    S = n_used.size
    given = rng.integers(0, n_used[None, :], (3, S))
    for lam in (0.0, 0.5):
        a = _device(eu, ev, g, d2, n_used, score, sweeps=5, damping=lam, candidates=given)
        b = _device(eu, ev, g, d2, n_used, score, sweeps=5, damping=lam, candidates=given)
        for name in EXACT + ("candidate_log_score", "log_score"):
            assert torch.equal(_bits(a[name]), _bits(b[name])), (lam, name)
        one = _device(eu, ev, g, d2, n_used, score, sweeps=5, damping=lam, candidates=given[:1])
        for name in ("candidate_state", "candidate_log_score", "refine_moves"):      # a candidate does not depend on how many there are
            assert one[name].shape[0] == 2 and torch.equal(_bits(one[name]), _bits(a[name][:2])), (lam, name)
        for name in ("max_marginal", "residual", "decoded_state"):
            assert torch.equal(_bits(one[name]), _bits(a[name])), (lam, name)
    flat = _device(eu, ev, g, d2, n_used, None, sweeps=5)                      # score None: zeros
    zeros = _device(eu, ev, g, d2, n_used, np.zeros((S, 130)), sweeps=5)
    assert torch.equal(_bits(flat["max_marginal"]), _bits(zeros["max_marginal"])) and torch.equal(flat["state"], zeros["state"])
    # refine alone: the rows of graph_path, one section or many, host or device states
    dev = _dev()
    t_d2, t_score = torch.as_tensor(d2).to(dev), torch.as_tensor(score).to(dev)
    many = sections.refine(given, t_d2, g, eu, ev, n_used, score=t_score, sweeps=16)
    ref = sections.refine_reference(given, eu, ev, g, d2, n_used, score=score, sweeps=16)
    assert np.array_equal(many["state"].cpu().numpy(), ref["state"]) and np.array_equal(many["refine_moves"].cpu().numpy(), ref["refine_moves"])
    assert torch.equal(many["state"], a["candidate_state"][1:]) and torch.equal(many["refine_moves"], a["refine_moves"][1:])
    single = sections.refine(torch.as_tensor(given[2]).to(dev), t_d2, g, eu, ev, n_used, score=t_score)
    assert single["state"].shape == (S,) and single["refine_moves"].shape == (16,) and single["log_score"].ndim == 0
    assert torch.equal(single["state"], many["state"][2]) and torch.equal(_bits(single["log_score"]), _bits(many["log_score"][2]))
    before = sections.graph_log_score(torch.as_tensor(given).to(dev).int(), t_score, torch.as_tensor(g).to(dev), t_d2, torch.as_tensor(eu).to(dev),
                                      torch.as_tensor(ev).to(dev))
    assert bool((many["log_score"] >= before).all()) and bool((many["refine_moves"].sum(dim=1) > 0).all())
    still = sections.refine(many["state"], t_d2, g, eu, ev, n_used, score=t_score, sweeps=2)      # a local mode stays
    assert torch.equal(still["state"], many["state"]) and bool((still["refine_moves"] == 0).all())


@pytest.mark.parametrize("name,diameter", [("line", 5), ("star", 3)])
def test_a_tree_converges_in_its_diameter(name, diameter):
    rng = np.random.default_rng(5 + diameter)
    eu, ev, n_used = _graph(name, 65, rng)
    score, g, d2 = _inputs(rng, eu, ev, n_used, 65)
    got = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=diameter + 3))
    print(name, "residual", got["residual"])
    assert np.all(got["residual"][diameter:] == 0.0) and np.all(got["residual"][:2] > 0.0) and np.all(got["refine_moves"] == 0)
    again = _numpy(_device(eu, ev, g, d2, n_used, score, sweeps=diameter))
    assert np.array_equal(again["max_marginal"], got["max_marginal"]) and np.array_equal(again["state"], got["state"])


def test_the_c_entries_refuse_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    S, E, n, sweeps, C, refine = 3, 2, 4, 2, 2, 3
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)      # noqa: E731
    host = lambda v: np.ctypeslib.as_ctypes(np.array(v, dtype=np.int32))      # noqa: E731
    eu, ev, nu, in_ptr, in_edge = i32([0, 1]), i32([1, 2]), i32([4, 4, 4]), i32([0, 1, 3, 4]), i32([1, 0, 3, 2])
    score, g, d2, msg, resid, mm, residual = f64(S, n), f64(E), f64(E, n, n), f64(2, 2 * E, n), f64(sweeps, 2 * E), f64(S, n), f64(sweeps)
    level, node, decoded = i32([0, 1, 2]), i32([0, 1, 2]), torch.full((S,), 7, dtype=torch.int32, device=dev)
    state, moves = torch.full((C, S), 7, dtype=torch.int32, device=dev), torch.full((C, refine), 7, dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else a.data_ptr()                          # noqa: E731
    path = lambda S_=S, E_=E, n_=n, eu_=eu, ev_=ev, nu_=nu, score_=score, g_=g, d2_=d2, ptr_=in_ptr, edge_=in_edge, sweeps_=sweeps, lam=0.0, levels=3, \
        lp=host([0, 1, 2, 3]), node_=node, level_=level, msg_=msg, resid_=resid, mm_=mm, decoded_=decoded, residual_=residual: \
        lib.gbp_section_graph_path(S_, E_, n_, p(eu_), p(ev_), p(nu_), p(score_), p(g_), p(d2_), p(ptr_), p(edge_), sweeps_, lam, levels, lp, p(node_), p(level_),
                                   p(msg_), p(resid_), p(mm_), p(decoded_), p(residual_), st)     # noqa: E731
    for kw in (dict(S_=-1), dict(E_=-1), dict(E_=2 ** 30), dict(n_=0), dict(n_=257), dict(sweeps_=0), dict(lam=1.0), dict(lam=-0.5), dict(lam=float("nan")),
               dict(S_=1), dict(S_=2 ** 31 - 1, E_=2 ** 29), dict(levels=0), dict(levels=4), dict(lp=None), dict(lp=host([1, 1, 2, 3])), dict(lp=host([0, 2, 1, 3])),
               dict(lp=host([0, 1, 2, 2])), dict(eu_=None), dict(ev_=None), dict(nu_=None), dict(score_=None), dict(g_=None), dict(d2_=None), dict(ptr_=None),
               dict(edge_=None), dict(node_=None), dict(level_=None), dict(msg_=None), dict(resid_=None), dict(mm_=None), dict(decoded_=None),
               dict(residual_=None)):
        assert path(**kw) != 0 and b"gbp_section_graph_path" in lib.gbp_last_error(), kw
    again = lambda S_=S, E_=E, n_=n, C_=C, eu_=eu, ev_=ev, nu_=nu, score_=score, g_=g, d2_=d2, ptr_=in_ptr, edge_=in_edge, colours=2, cp=host([0, 2, 3]), \
        node_=node, refine_=refine, state_=state, moves_=moves: \
        lib.gbp_section_graph_refine(S_, E_, n_, C_, p(eu_), p(ev_), p(nu_), p(score_), p(g_), p(d2_), p(ptr_), p(edge_), colours, cp, p(node_), refine_,
                                     p(state_), p(moves_), st)                 # noqa: E731
    for kw in (dict(S_=-1), dict(E_=-1), dict(E_=2 ** 30), dict(n_=0), dict(n_=257), dict(C_=0), dict(C_=65538), dict(refine_=-1), dict(refine_=65537),
               dict(S_=1), dict(S_=2 ** 31 - 1, E_=2 ** 29), dict(S_=2 ** 30, C_=4), dict(colours=0), dict(colours=4), dict(cp=None), dict(cp=host([1, 2, 3])),
               dict(cp=host([0, 3, 2])), dict(cp=host([0, 2, 2])), dict(eu_=None), dict(ev_=None), dict(nu_=None), dict(score_=None), dict(g_=None),
               dict(d2_=None), dict(ptr_=None), dict(edge_=None), dict(node_=None), dict(state_=None), dict(moves_=None)):
        assert again(**kw) != 0 and b"gbp_section_graph_refine" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    for t in (msg, resid, mm, residual):
        assert bool((t == 7.0).all())                                          # nothing was written
    assert bool((decoded == 7).all()) and bool((state == 7).all()) and bool((moves == 7).all())
    assert path(S_=0, E_=0) == 0 and again(S_=0, E_=0) == 0 and again(refine_=0) == 0      # nothing to do: no launch
    torch.cuda.synchronize()
    assert bool((residual == 7.0).all()) and bool((moves == 7).all())
    none = sections.graph_path(torch.zeros((0, 4, 4), dtype=torch.float64, device=dev), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                               np.zeros(0, dtype=np.int32), 0, sweeps=3)
    assert none["state"].shape == (0,) and none["max_marginal"].shape == (0, 4) and bool((none["residual"] == 0.0).all()) and none["refine_moves"].shape == (1, 16)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

def _planted():
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    return _to_device(k, edges, sigma), edges, x, y, ptr, truth


def test_spatial_adds_the_path_and_changes_nothing_else():
    ens, edges, x, y, ptr, truth = _planted()
    S, n = ens.k.shape
    middle = np.arange(S_LINES, 2 * S_LINES)
    kw = dict(ptr=ptr, max_models=n, max_distance=1.5 * SPACING)
    plain = _numpy(sections.spatial(ens, x, y, Z1_LINES, **kw))
    none = _numpy(sections.spatial(ens, x, y, Z1_LINES, path=None, **kw))
    got = _numpy(sections.spatial(ens, x, y, Z1_LINES, path=True, **kw))
    new = {"path_state", "path_slot", "path_k", "path_edges", "path_sigma", "path_log_score", "state_log_score", "path_margin", "path_residual",
           "path_candidate_log_score", "path_chosen", "path_edge_distance"}
    assert set(none) == set(plain) and set(got) == set(plain) | new
    for name in plain:                                                         # every present output keeps its bits
        for other in (none, got):
            assert other[name].dtype == plain[name].dtype and np.array_equal(other[name], plain[name], equal_nan=plain[name].dtype.kind == "f"), name
    # the rule on the device's own distances
    eu, ev, g, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * SPACING)
    d2 = sections.edge_distance(ens, torch.as_tensor(got["rows"]).to(_dev()), eu, ev, 0.0, Z1_LINES).cpu().numpy()
    ref = sections.graph_path_reference(eu, ev, g, d2, got["n_used"], None, candidates=got["state"][None, :])
    assert np.array_equal(got["path_state"], ref["state"]) and np.array_equal(got["path_residual"], ref["residual"]) and int(got["path_chosen"]) == ref["chosen"]
    assert np.allclose(got["path_candidate_log_score"], ref["candidate_log_score"], rtol=0, atol=1e-11)
    two = np.sort(ref["max_marginal"], axis=1)[:, -2:]
    assert np.array_equal(got["path_margin"], two[:, 1] - two[:, 0]) and np.all(got["path_margin"] >= 0.0)
    print("planted lines on the device: the belief argmax scores %.3f, the path %.3f; %d soundings differ"
          % (got["state_log_score"], got["path_log_score"], int((got["path_state"] != got["state"]).sum())))
    assert got["path_log_score"] > got["state_log_score"] and got["path_log_score"] == got["path_candidate_log_score"].max()
    assert np.all(got["path_state"][middle] >= 10) and np.all(np.abs(edges[np.arange(S), got["path_state"], 0] - truth) <= 4.0)
    assert np.array_equal(got["path_slot"], got["path_state"]) and np.array_equal(got["path_edges"], edges[np.arange(S), got["path_state"]])
    assert np.array_equal(got["path_edge_distance"], np.sqrt(d2[np.arange(eu.size), got["path_state"][eu], got["path_state"][ev]]))
    # with draws the best realisation is a candidate: the path is never less probable than any of them
    drawn = _numpy(sections.spatial(ens, x, y, Z1_LINES, path=dict(sweeps=16, refine=8), draws=64, seed=3, **kw))
    assert drawn["path_candidate_log_score"].shape == (3,) and drawn["path_residual"].shape == (16,)
    assert drawn["path_log_score"] >= drawn["draw_log_score"].max() and drawn["path_log_score"] >= drawn["state_log_score"]
    # a sounding without models is left out of the graph
    kk = ens.k.clone()
    kk[9] = 0
    cut = _numpy(sections.spatial(ens._replace(k=kk), x, y, Z1_LINES, path=True, **kw))
    assert cut["path_state"][9] == -1 and cut["path_slot"][9] == -1 and np.isnan(cut["path_margin"][9]) and cut["path_k"][9] == 0
    assert np.all(cut["path_state"][np.arange(S) != 9] >= 0) and cut["path_log_score"] >= cut["state_log_score"]


def test_from_survey_and_the_command_line(tmp_path):
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    survey = dict(ensemble_k=k, ensemble_edges=edges, ensemble_sigma=sigma, line=np.repeat([10, 20, 30], S_LINES), x=x, y=y, fiducial=np.arange(k.shape[0]))
    direct = _numpy(sections.spatial_from_survey(survey, Z1_LINES, max_models=16, max_distance=150.0, sweeps=12, path=dict(sweeps=12)))
    both = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, spatial=dict(max_models=16, max_distance=150.0, sweeps=12, path=dict(sweeps=12))))
    assert {"path_state", "path_log_score", "path_margin", "path_edge_distance"} <= set(direct) and direct["path_residual"].shape == (12,)
    for name in direct:
        if name not in ("line", "fiducial", "x", "y"):
            assert np.array_equal(both["spatial_" + name], direct[name], equal_nan=True), name
    path = str(tmp_path / "survey.npz")
    np.savez(path, **survey)
    written = sections.main([path, "--depth", "120", "--spatial", "150", "--sweeps", "12", "--max-models", "16", "--path", "12"])
    f = sections.load(written)
    assert set(f) == set(direct) and all(np.array_equal(f[name], direct[name], equal_nan=True) for name in direct)
