"""Horizons across flight lines on the device (csrc/gbp_horizon_graph.h k_hgraph_init / k_hgraph_sweep / k_hgraph_node /
k_hgraph_condition through gbp_horizon_graph_propagate, gbp_horizon_graph_path and gbp_horizon_graph_refine; geobipy_amd.horizons
propagate, graph_path, refine, spatial, spatial_from_products).

The max-sum side is held to ``horizons.graph_path_reference`` with ``==``: there is no exp and no reordered operation.  The sum side
is held to ``horizons.propagate_reference`` in fp64: belief and residual within 16 max(e, U), e the fp64 rule's own distance from the
rule in long double, measured per case, and U = 2^-53 (the bar of test_spatial_sections_gpu.py); NaN where the rule has NaN; ``state``
the first maximum of the device's own belief.  Every case prints used / bound."""
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, horizons, sections
from test_horizon_graph import DECOY_CELLS, PER_LINE, U, horizon_inputs, planted_horizon
from test_spatial_sections import lattice_graph, line_graph, star_graph

SURVEY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_survey_0.0.h5")
SWITCH = 2.3
GRAPHS = ("line", "star", "lattice", "isolated")
PATH_EXACT = ("max_marginal", "residual", "decoded_state", "state", "log_score", "refine_moves", "candidate_state", "candidate_log_score", "chosen")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _on(score, ab):
    return torch.as_tensor(score).to(_dev()), None if ab is None else torch.as_tensor(ab).to(_dev())


def _graph(name):
    if name == "line":
        eu, ev, nu = line_graph()
        return eu, ev, nu.size
    if name == "star":
        eu, ev, nu = star_graph()
        return eu, ev, nu.size
    if name == "lattice":
        return lattice_graph()
    return np.array([0, 0, 1, 3]), np.array([1, 3, 4, 4]), 6                   # sounding 2 has no edge; 5 neither, at the end


def _same_path(got, ref, what):
    for name in PATH_EXACT:
        assert np.array_equal(_bits(got[name]), _bits(np.asarray(ref[name], dtype=got[name].dtype))), (what, name)


@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("name", GRAPHS)
def test_the_device_against_the_rules(name, S, absent):
    rng = np.random.default_rng(1000 * GRAPHS.index(name) + 2 * S + absent)
    eu, ev, N = _graph(name)
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, absent)
    t_score, t_ab = _on(score, ab)
    SA = S + absent
    given = rng.integers(0, SA, (1, N))
    for sweeps in (1, 2, 7):
        for lam in (0.0, 0.5):
            kw = dict(sweeps=sweeps, damping=lam)
            # max-sum: the rule's bits
            got = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, t_ab, refine=4, candidates=given, **kw))
            ref = horizons.graph_path_reference(eu, ev, g, d, dz, SWITCH, score, ab, refine=4, candidates=given, **kw)
            assert got["max_marginal"].shape == (N, SA) and got["state"].dtype == np.int32 and got["refine_moves"].shape == (2, 4)
            _same_path(got, ref, kw)
            # sum-product: the reference's own rounding
            got = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, t_ab, **kw))
            ref = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, **kw)
            ld = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, dtype=np.longdouble, **kw)
            assert got["belief"].shape == (N, SA) and got["belief"].dtype == np.float64 and got["state"].dtype == np.int32 and got["residual"].shape == (sweeps,)
            assert np.all(np.isfinite(ref["belief"])) and np.all(np.isfinite(ref["residual"]))
            assert np.all(np.isfinite(got["belief"])) and np.all(np.isfinite(got["residual"]))
            e_b, e_r = float(np.abs(ref["belief"] - ld["belief"]).max()), float(np.abs(ref["residual"] - ld["residual"]).max())
            b_b, b_r = 16.0 * max(e_b, U), 16.0 * max(e_r, U)
            d_b, d_r = float(np.abs(got["belief"] - ref["belief"]).max()), float(np.abs(got["residual"] - ref["residual"]).max())
            print("%s S=%d absent=%s sweeps=%d damping=%.1f: belief e=%.3g used/bound %.3f; residual e=%.3g used/bound %.3f"
                  % (name, S, absent, sweeps, lam, e_b, d_b / b_b, e_r, d_r / b_r))
            assert d_b <= b_b
            assert d_r <= b_r
            for s in range(N):
                assert got["state"][s] == sections.first_max(got["belief"][s])
            assert float(np.abs(got["belief"].sum(axis=1) - 1.0).max()) <= b_b + 4 * U * SA
    if name == "isolated":                                                     # no edges: the normalised w
        theta = score if ab is None else np.concatenate([score, ab[:, None]], axis=1)
        for s in (2, 5):
            w = np.exp(theta[s])
            assert float(np.abs(got["belief"][s] - w / w.sum()).max()) <= 16.0 * U


@pytest.mark.parametrize("absent", [False, True])
def test_the_largest_state_count(absent):
    """S = 2048: the LDS limit (65 552 B of dynamic LDS) and nine owned states a thread, on a path of 3 soundings with 2 sweeps."""
    S, N = 2048, 3
    rng = np.random.default_rng(2048 + absent)
    eu, ev = np.array([0, 1]), np.array([1, 2])
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, absent, slope=2.0)
    t_score, t_ab = _on(score, ab)
    got = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=2, refine=2))
    ref = horizons.graph_path_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2, refine=2)
    _same_path(got, ref, "S = 2048")
    got = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=2))
    ref = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2)
    ld = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2, dtype=np.longdouble)
    e_b, e_r = float(np.abs(ref["belief"] - ld["belief"]).max()), float(np.abs(ref["residual"] - ld["residual"]).max())
    b_b, b_r = 16.0 * max(e_b, U), 16.0 * max(e_r, U)
    d_b, d_r = float(np.abs(got["belief"] - ref["belief"]).max()), float(np.abs(got["residual"] - ref["residual"]).max())
    print("S=2048 absent=%s: belief e=%.3g used/bound %.3f; residual e=%.3g used/bound %.3f" % (absent, e_b, d_b / b_b, e_r, d_r / b_r))
    assert np.all(np.isfinite(got["belief"])) and d_b <= b_b
    assert d_r <= b_r
    assert all(got["state"][s] == sections.first_max(got["belief"][s]) for s in range(N))


@pytest.mark.parametrize("S", [127, 128, 255, 256, 513, 769, 1025, 1281, 1537, 1793])
def test_every_instance_of_the_sweep(S):
    """With the absent state SA = S + 1 = 128 is the last state count a half of the workgroup takes (SPLIT), 129 and 256 the first and
    the last with one owned state a thread, and 257, 514, .. 1 794 the first with 2, 3, .. 8: every instance between those the other
    tests launch, on a path of 3 soundings with 2 sweeps."""
    rng = np.random.default_rng(S)
    eu, ev = np.array([0, 1]), np.array([1, 2])
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, 3, S, True, slope=2.0)
    t_score, t_ab = _on(score, ab)
    for lam in (0.0, 0.5):
        got = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=2, damping=lam, refine=2))
        _same_path(got, horizons.graph_path_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2, damping=lam, refine=2), (S, lam))
        got = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=2, damping=lam))
        ref = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2, damping=lam)
        ld = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, ab, sweeps=2, damping=lam, dtype=np.longdouble)
        e_b, e_r = float(np.abs(ref["belief"] - ld["belief"]).max()), float(np.abs(ref["residual"] - ld["residual"]).max())
        b_b, b_r = 16.0 * max(e_b, U), 16.0 * max(e_r, U)
        d_b, d_r = float(np.abs(got["belief"] - ref["belief"]).max()), float(np.abs(got["residual"] - ref["residual"]).max())
        print("S=%d damping=%.1f: belief e=%.3g used/bound %.3f; residual e=%.3g used/bound %.3f" % (S, lam, e_b, d_b / b_b, e_r, d_r / b_r))
        assert np.all(np.isfinite(got["belief"])) and d_b <= b_b
        assert d_r <= b_r
        assert all(got["state"][s] == sections.first_max(got["belief"][s]) for s in range(3))


def test_nan_where_the_rule_has_nan():
    eu, ev, _ = star_graph()
    score, _, g, d, dz = horizon_inputs(np.random.default_rng(4), eu, ev, 5, 3, False)
    g[3], d[3] = 1e6, 0.3 * dz                                                 # the tail's K underflows: its messages are 0 / 0
    t_score, _ = _on(score, None)
    for sweeps in (1, 3):
        got = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, None, sweeps=sweeps))
        ref = horizons.propagate_reference(eu, ev, g, d, dz, SWITCH, score, None, sweeps=sweeps)
        assert np.isnan(ref["belief"]).any() and np.isnan(ref["residual"]).all()
        assert np.array_equal(np.isnan(got["belief"]), np.isnan(ref["belief"])) and np.array_equal(np.isnan(got["residual"]), np.isnan(ref["residual"]))
        ok = ~np.isnan(ref["belief"])
        assert float(np.abs(got["belief"][ok] - ref["belief"][ok]).max(initial=0.0)) <= 16.0 * U * 4
        assert np.array_equal(got["state"], ref["state"])                      # a NaN never replaces the first state
    got = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, None, sweeps=3))      # the log domain does not underflow
    _same_path(got, horizons.graph_path_reference(eu, ev, g, d, dz, SWITCH, score, None, sweeps=3), "g = 1e6")


def test_a_call_repeats_its_own_bits():
    rng = np.random.default_rng(77)
    eu, ev, N = lattice_graph()
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, 300, True)
    t_score, t_ab = _on(score, ab)
    for lam in (0.0, 0.5):
        a = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=5, damping=lam))
        b = _numpy(horizons.propagate(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=5, damping=lam))
        for name in ("belief", "state", "residual"):
            assert np.array_equal(_bits(a[name]), _bits(b[name])), (lam, name)
        a = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=5, damping=lam))
        b = _numpy(horizons.graph_path(eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=5, damping=lam))
        for name in PATH_EXACT:
            assert np.array_equal(_bits(a[name]), _bits(b[name])), (lam, name)


@pytest.mark.parametrize("absent", [False, True])
def test_refine_from_a_random_start(absent):
    rng = np.random.default_rng(31 + absent)
    eu, ev, N = lattice_graph()
    S = 70
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, absent)
    t_score, t_ab = _on(score, ab)
    start = rng.integers(0, S + absent, (3, N))
    got = _numpy(horizons.refine(start, eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=6))
    ref = horizons.refine_reference(start, eu, ev, g, d, dz, SWITCH, score, ab, sweeps=6)
    assert ref["refine_moves"][:, 0].min() > 0                                 # a random start moves
    for name in ("state", "refine_moves", "log_score"):
        assert np.array_equal(_bits(got[name]), _bits(np.asarray(ref[name], dtype=got[name].dtype))), name
    before = horizons.graph_log_score(start, eu, ev, g, d, dz, SWITCH, score, ab)
    assert np.all(got["log_score"] > before)
    one = _numpy(horizons.refine(torch.as_tensor(start[1]).to(_dev()), eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=6))
    assert np.array_equal(one["state"], got["state"][1]) and one["refine_moves"].shape == (6,) and one["log_score"] == got["log_score"][1]
    same = _numpy(horizons.refine(start, eu, ev, g, d, dz, SWITCH, t_score, t_ab, sweeps=0))
    assert np.array_equal(same["state"], start) and same["refine_moves"].shape == (3, 0)


def test_the_planted_lines_through_spatial():
    evidence, x, y, surface, edges, ptr, cell = planted_horizon()
    middle = np.arange(PER_LINE, 2 * PER_LINE)
    e = torch.as_tensor(evidence).to(_dev())
    out = _numpy(horizons.spatial(e, x, y, surface, edges, max_distance=150.0, ptr=ptr, sweeps=16))
    track = _numpy(horizons.track(e, x, y, surface, edges, ptr=ptr))
    assert {k for k in track if k not in ("log_partition", "scale")} <= set(out)
    assert out["edge_u"].size == 57 and out["residual"].shape == (16,) and out["path_residual"].shape == (16,)
    assert np.array_equal(out["line_cell"], track["cell"]) and np.array_equal(out["line_cell"][middle], cell[middle] + DECOY_CELLS)      # 12 of 12 on the decoy
    assert np.array_equal(out["cell"], cell) and np.array_equal(out["belief_cell"], cell)                                                # 36 of 36 on the horizon
    assert np.array_equal(out["depth"], cell + 0.5) and np.array_equal(out["elevation"], surface - (cell + 0.5))
    assert out["marginal"].shape == (36, 64) and np.all(out["absent_probability"] == 0.0)
    assert np.all(out["depth_percentile_5"] <= out["depth_percentile_50"]) and np.all(out["depth_percentile_50"] <= out["depth_percentile_95"])
    assert out["path_candidate_log_score"].shape == (3,) and out["log_score"] == out["path_candidate_log_score"][out["path_chosen"]]
    assert out["log_score"] >= out["path_candidate_log_score"].max() and out["state_log_score"] == out["log_score"] and np.all(out["path_margin"] > 0.0)
    eu, ev, _, dist = sections.neighbours(x, y, ptr, None, max_distance=150.0)
    assert np.array_equal(out["edge_u"], eu) and np.array_equal(out["edge_v"], ev) and np.array_equal(out["edge_length"], dist)
    # the rules on the device's own scores
    score = horizons.evidence_scores(e)[0].cpu().numpy()
    g, d, _ = horizons.graph_steps(x, y, surface, eu, ev)
    rule = horizons.propagate_reference(eu, ev, g, d, 1.0, 4.6, score, None, sweeps=16)
    assert np.allclose(out["marginal"], rule["belief"], rtol=0, atol=1e-13)
    path = horizons.graph_path_reference(eu, ev, g, d, 1.0, 4.6, score, None, sweeps=16, candidates=np.stack([out["belief_cell"], out["line_cell"]]))
    assert np.array_equal(out["cell"], path["state"]) and out["log_score"] == path["log_score"]
    assert np.array_equal(out["path_candidate_log_score"], path["candidate_log_score"])
    # a window, the absent state, and the beliefs alone
    ab = torch.full((36,), 0.05, dtype=torch.float64, device=_dev())
    win = _numpy(horizons.spatial(e, x, y, surface, edges, max_distance=150.0, ptr=ptr, sweeps=16, between=(8.0, 40.0), absent=ab, path=False))
    assert np.array_equal(win["cell"], cell) and win["marginal"].shape == (36, 32) and np.all(win["absent_probability"] < 1e-3)
    assert "path_margin" not in win and np.array_equal(win["cell"], win["belief_cell"]) and win["log_score"] == win["state_log_score"]
    # no edge across the lines: every line alone, the chain's marginals and its Viterbi path
    alone = _numpy(horizons.spatial(e, x, y, surface, edges, max_distance=50.0, ptr=ptr, sweeps=12))
    assert alone["edge_u"].size == 33 and alone["residual"][11] == 0.0 and np.array_equal(alone["cell"], track["cell"])
    assert np.allclose(alone["marginal"], track["marginal"], rtol=0, atol=1e-12)


def test_the_command_line_on_copies_of_a_container(tmp_path):
    for name in ("0.0.h5", "1.0.h5"):                                          # two lines (at the same places: the cross edges are clamped)
        shutil.copy(SURVEY, str(tmp_path / name))
    written = horizons.main([str(tmp_path), "--between", "5", "60", "--between", "20", "100", "--spatial", "10", "--sweeps", "6"])
    assert written == [str(tmp_path / "survey.horizons.npz")] and os.path.exists(written[0])
    f = horizons.load(written[0])
    N = 16
    assert f["cell"].shape == (2, N) and f["line_cell"].shape == (2, N) and f["residual"].shape == (2, 6) and f["log_score"].shape == (2,)
    assert f["marginal_0"].shape == (N, 110) and f["marginal_1"].shape == (N, 160) and np.array_equal(f["ptr"], [0, 8, 16])
    assert f["edge_u"].size == 14 + 8 and np.array_equal(f["between"], [[5.0, 60.0], [20.0, 100.0]])
    assert np.all((f["depth"][0] >= 5.0) & (f["depth"][0] < 60.0)) and np.all((f["depth"][1] >= 20.0) & (f["depth"][1] < 100.0))
    direct = _numpy(horizons.spatial_from_products([str(tmp_path / "0.0.h5"), str(tmp_path / "1.0.h5")], [(5.0, 60.0), (20.0, 100.0)], 10.0, sweeps=6))
    assert set(direct) == set(f) and all(np.array_equal(direct[k], f[k], equal_nan=True) for k in f)
    plain = horizons.main([str(tmp_path / "0.0.h5"), "--between", "5", "60", "--no-marginals"])      # without --spatial nothing changes
    assert plain == [str(tmp_path / "0.0.horizons.npz")]


def test_the_c_entries_refuse_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    N, E, S, sweeps, C, refine = 3, 2, 4, 2, 2, 2
    SA = S + 1
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)      # noqa: E731
    p = lambda a: None if a is None else a.data_ptr()                          # noqa: E731
    host = lambda v: None if v is None else np.ctypeslib.as_ctypes(np.asarray(v, dtype=np.int32))      # noqa: E731
    base = dict(N=N, E=E, S=S, absent=1, dz=0.5, sw=2.0, eu=i32([0, 1]), ev=i32([1, 2]), score=f64(N, SA), g=f64(E), d=f64(E), ptr=i32([0, 1, 3, 4]),
                edge=i32([1, 0, 3, 2]), sweeps=sweeps, lam=0.0)
    shared = (dict(N=-1), dict(E=-1), dict(E=2 ** 30), dict(S=0), dict(S=2049), dict(absent=2), dict(dz=0.0), dict(dz=float("nan")), dict(sw=-1.0),
              dict(sw=float("inf")), dict(N=1), dict(N=2 ** 31 - 1, E=2 ** 29), dict(eu=None), dict(ev=None), dict(score=None), dict(g=None), dict(d=None),
              dict(ptr=None), dict(edge=None))
    swept = (dict(sweeps=0), dict(lam=1.0), dict(lam=-0.5), dict(lam=float("nan")), dict(E=2 ** 29, sweeps=2 ** 31 - 1))

    outs = dict(w=f64(N, SA), mu=f64(2, 2 * E, SA), resid=f64(sweeps, 2 * E), belief=f64(N, SA), state=i32([7] * N), residual=f64(sweeps))

    def propagate(**kw):
        a = {**base, **outs, **kw}
        return lib.gbp_horizon_graph_propagate(a["N"], a["E"], a["S"], a["absent"], a["dz"], a["sw"], p(a["eu"]), p(a["ev"]), p(a["score"]), p(a["g"]), p(a["d"]),
                                               p(a["ptr"]), p(a["edge"]), a["sweeps"], a["lam"], p(a["w"]), p(a["mu"]), p(a["resid"]), p(a["belief"]),
                                               p(a["state"]), p(a["residual"]), st)
    for kw in shared + swept + tuple({k: None} for k in outs):
        assert propagate(**kw) != 0 and b"gbp_horizon_graph_propagate" in lib.gbp_last_error(), kw

    levels = dict(n_levels=3, level_ptr=[0, 1, 2, 3], level_node=i32([0, 1, 2]), level=i32([0, 1, 2]))
    pouts = dict(nu=f64(2, 2 * E, SA), resid=f64(sweeps, 2 * E), max_marginal=f64(N, SA), decoded=i32([7] * N), residual=f64(sweeps))

    def path(**kw):
        a = {**base, **levels, **pouts, **kw}
        return lib.gbp_horizon_graph_path(a["N"], a["E"], a["S"], a["absent"], a["dz"], a["sw"], p(a["eu"]), p(a["ev"]), p(a["score"]), p(a["g"]), p(a["d"]),
                                          p(a["ptr"]), p(a["edge"]), a["sweeps"], a["lam"], a["n_levels"], host(a["level_ptr"]), p(a["level_node"]),
                                          p(a["level"]), p(a["nu"]), p(a["resid"]), p(a["max_marginal"]), p(a["decoded"]), p(a["residual"]), st)
    groups = (dict(n_levels=0), dict(n_levels=4), dict(level_ptr=None), dict(level_ptr=[1, 1, 2, 3]), dict(level_ptr=[0, 2, 1, 3]), dict(level_ptr=[0, 1, 2, 4]),
              dict(level_node=None), dict(level=None))
    for kw in shared + swept + groups + tuple({k: None} for k in pouts):
        assert path(**kw) != 0 and b"gbp_horizon_graph_path" in lib.gbp_last_error(), kw

    colours = dict(n_colours=2, colour_ptr=[0, 2, 3], colour_node=i32([0, 2, 1]), C=C, refine=refine)
    routs = dict(X=i32([[7] * N] * C), moves=i32([[7] * refine] * C))

    def ascent(**kw):
        a = {**base, **colours, **routs, **kw}
        return lib.gbp_horizon_graph_refine(a["N"], a["E"], a["S"], a["absent"], a["dz"], a["sw"], a["C"], p(a["eu"]), p(a["ev"]), p(a["score"]), p(a["g"]),
                                            p(a["d"]), p(a["ptr"]), p(a["edge"]), a["n_colours"], host(a["colour_ptr"]), p(a["colour_node"]), a["refine"],
                                            p(a["X"]), p(a["moves"]), st)
    groups = (dict(n_colours=0), dict(n_colours=4), dict(colour_ptr=None), dict(colour_ptr=[1, 2, 3]), dict(colour_ptr=[0, 3, 2]), dict(colour_ptr=[0, 2, 4]),
              dict(colour_node=None), dict(C=0), dict(C=65538), dict(refine=-1), dict(refine=65537), dict(N=2 ** 16, E=1, C=2 ** 15), dict(X=None),
              dict(moves=None))
    for kw in shared + groups:
        assert ascent(**kw) != 0 and b"gbp_horizon_graph_refine" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(pouts.values()) + list(routs.values()):
        assert bool((t == 7).all())                                            # nothing was written
    # nothing to read: no soundings, and soundings without a single edge
    none = np.zeros(0, dtype=np.int64)
    empty = horizons.propagate(none, none, np.zeros(0), np.zeros(0), 0.5, 2.0, torch.zeros((0, 4), dtype=torch.float64, device=dev), sweeps=3)
    assert empty["belief"].shape == (0, 4) and empty["state"].shape == (0,) and bool((empty["residual"] == 0.0).all())
    score = torch.tensor([[0.5, -1.0, 9.0, 2.0], [0.0, 1.0, 2.0, 3.0]], dtype=torch.float64, device=dev)
    apart = horizons.propagate(none, none, np.zeros(0), np.zeros(0), 0.5, 2.0, score, sweeps=3)
    w = np.exp(score.cpu().numpy())
    assert float(np.abs(apart["belief"].cpu().numpy() - w / w.sum(axis=1, keepdims=True)).max()) <= 16.0 * U
    assert apart["state"].tolist() == [2, 3] and bool((apart["residual"] == 0.0).all())
    found = horizons.graph_path(none, none, np.zeros(0), np.zeros(0), 0.5, 2.0, score, sweeps=3)
    assert found["state"].tolist() == [2, 3] and found["log_score"] == 12.0 and bool((found["residual"] == 0.0).all())
