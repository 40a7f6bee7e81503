"""Joint draws across flight lines on the device (csrc/gbp_section_graph_draw.h k_graph_weights / k_graph_line_filter /
k_graph_line_draw through gbp_section_graph_draw; geobipy_amd.sections graph_draw, propagate(keep_kernel=), spatial(draws=); DESIGN.md
3.29), held to ``sections.graph_draw_reference``.

The bounds are those of test_section_draws_gpu.py.  ``draw_state`` equals the fp64 rule's with ``==`` in every realisation whose
margin is at least 1e-9 at every sounding and sweep -- a whole realisation is left out otherwise, because lines talk to each other; a
decision falls within 1e-9 of one of m boundaries with probability about 2 m 1e-9, far below one realisation per case, at most 1 % may
be left out, and every case prints the count.  ``filtered`` of those realisations lies within max(16 e, 16 * 2^-52) of the long-double
rule, e the fp64 rule's own distance from it, and n * bound <= 1e-10 is asserted, so the close-call threshold stands well above what
the filter's rounding can move a cumulative sum."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, sections
from test_families_gpu import _to_device
from test_section_draws import R_STAT
from test_spatial_draws import LADDER_SEED, LADDER_SWEEPS, check_ladder, ladder_case, true_share
from test_spatial_sections import S_LINES, SPACING, Z1_LINES, graph_inputs, lattice_graph, line_graph, planted_lines, star_graph

U = 2.0 ** -52
CLOSE = 1.0e-9


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _case(name, n, seed):
    """(eu, ev, g, d2, n_used, score, ptr): a graph with its sequences and a ragged n_used that holds 1 and n.
    line: one sequence of six; cut: the same line as sequences of 1, 2 and 3 soundings (two cross edges); star: five singletons (two
    colours); lattice: 3 lines of 4; isolated: two soundings without an edge and an empty sequence; triangle: three sequences that all
    touch (a third colour)."""
    rng = np.random.default_rng(seed)
    if name in ("line", "cut"):
        eu, ev, nu = line_graph()
        S, ptr = nu.size, [0, 6] if name == "line" else [0, 1, 3, 6]
    elif name == "star":
        eu, ev, nu = star_graph()
        S, ptr = nu.size, np.arange(6)
    elif name == "lattice":
        eu, ev, S = lattice_graph()
        ptr = [0, 4, 8, 12]
    elif name == "isolated":
        eu, ev, S, ptr = np.array([0, 0, 1, 3]), np.array([1, 3, 4, 4]), 6, [0, 2, 3, 3, 5, 6]
    else:
        eu, ev, S, ptr = np.array([0, 0, 1, 2, 3]), np.array([1, 2, 4, 3, 4]), 5, [0, 2, 4, 5]
    n_used = rng.integers(1, n + 1, S)
    n_used[0], n_used[S - 2] = n, 1
    score, g, d2 = graph_inputs(rng, eu, ev, n_used, n)
    return eu, ev, g, d2, n_used, score, np.asarray(ptr)


def _device(case, R, **kw):
    eu, ev, g, d2, n_used, score, ptr = case
    dev = _dev()
    out = sections.graph_draw(torch.as_tensor(d2).to(dev), g, eu, ev, n_used, ptr, R, score=torch.as_tensor(score).to(dev), **kw)
    torch.cuda.synchronize()
    return out


def _rule(case, R, **kw):
    eu, ev, g, d2, n_used, score, ptr = case
    return sections.graph_draw_reference(eu, ev, g, d2, n_used, ptr, R, score=score, **kw)


def _check_against_the_rule(got, case, R, what, **kw):
    """``got`` (numpy) against the fp64 rule and the long-double rule, as the module's docstring says."""
    n_used, n = case[4], case[3].shape[1]
    S = n_used.size
    ref, ld = _rule(case, R, **kw), _rule(case, R, dtype=np.longdouble, **kw)
    keep = (ref["margin"] >= CLOSE).all(axis=1)
    left = int((~keep).sum())
    e = float(np.abs(ref["filtered"][keep] - ld["filtered"][keep]).max(initial=0.0))
    bound = max(16.0 * e, 16.0 * U)
    dist = float(np.abs(got["filtered"][keep] - ld["filtered"][keep]).max(initial=0.0))
    print("%s: %d of %d realisations left out (smallest margin %.3g); filter e=%.3g bound=%.3g device distance=%.3g"
          % (what, left, R, float(ref["margin"].min(initial=1.0)), e, bound, dist))
    assert left <= 0.01 * R
    assert np.array_equal(ld["draw_state"][keep], ref["draw_state"][keep])     # the yardstick walks the same way where nothing is close
    assert got["draw_state"].dtype == np.int32 and got["draw_state"].shape == (R, S) and got["filtered"].shape == (R, S, n)
    assert np.array_equal(got["draw_state"][keep], ref["draw_state"][keep])
    assert np.all(np.isfinite(ld["filtered"].astype(np.float64))) and dist <= bound
    assert n * bound <= 1.0e-10
    assert np.all(got["draw_state"] >= 0) and np.all(got["draw_state"] < n_used[None, :])
    for s in range(S):
        assert np.all(got["filtered"][:, s, n_used[s]:] == 0.0)


CASES = [("line", 1, 5, 1), ("line", 65, 64, 0), ("cut", 3, 65, 3), ("star", 63, 130, 1), ("lattice", 64, 65, 3), ("lattice", 130, 5, 1),
         ("isolated", 65, 64, 3), ("isolated", 3, 5, 0), ("triangle", 3, 130, 3), ("triangle", 130, 64, 1)]


@pytest.mark.parametrize("name,n,R,sweeps", CASES)
def test_draws_against_the_rule(name, n, R, sweeps):
    case = _case(name, n, 100 * n + R + sweeps)
    key = (3 * np.arange(case[4].size) + (np.arange(case[4].size) % 2) * 2 ** 40).astype(np.int64)
    got = _numpy(_device(case, R, seed=2 ** 35 + 7, sweeps=sweeps, row_key=key))
    _check_against_the_rule(got, case, R, "%s n=%d R=%d sweeps=%d" % (name, n, R, sweeps), seed=2 ** 35 + 7, sweeps=sweeps, row_key=key)


def test_what_a_draw_depends_on():
    case = _case("lattice", 65, 9)
    eu, ev, g, d2, n_used, score, ptr = case
    a, b = (_device(case, 65, seed=2 ** 40 + 9, sweeps=3) for _ in range(2))
    assert torch.equal(a["draw_state"], b["draw_state"]) and torch.equal(_bits(a["filtered"]), _bits(b["filtered"]))      # a call repeats its bits
    one = _device(case, 1, seed=2 ** 40 + 9, sweeps=3)
    assert torch.equal(one["draw_state"][0], a["draw_state"][0]) and torch.equal(_bits(one["filtered"][0]), _bits(a["filtered"][0]))
    assert not torch.equal(_device(case, 65, seed=9, sweeps=3)["draw_state"], a["draw_state"])      # the seed's high word is used
    two = _device(case, 65, seed=2 ** 40 + 9, sweeps=3, block=33)              # two blocks of realisations
    assert torch.equal(two["draw_state"], a["draw_state"]) and torch.equal(_bits(two["filtered"]), _bits(a["filtered"]))
    small = _device(case, 65, seed=2 ** 40 + 9, sweeps=3, budget_bytes=12 * 65 * 8 * 7, filtered=False)
    assert "filtered" not in small and torch.equal(small["draw_state"], a["draw_state"])
    dev = _dev()
    prop = sections.propagate(torch.as_tensor(d2).to(dev), g, eu, ev, n_used, n_used.size, score=torch.as_tensor(score).to(dev), sweeps=2, keep_kernel=True)
    plain = sections.propagate(torch.as_tensor(d2).to(dev), g, eu, ev, n_used, n_used.size, score=torch.as_tensor(score).to(dev), sweeps=2)
    assert set(prop) == set(plain) | {"kernel"} and all(torch.equal(_bits(prop[name]), _bits(plain[name])) for name in plain)
    ready = _device(case, 65, seed=2 ** 40 + 9, sweeps=3, kernel=prop["kernel"])
    assert torch.equal(ready["draw_state"], a["draw_state"]) and torch.equal(_bits(ready["filtered"]), _bits(a["filtered"]))
    first = _device(case, 65, seed=2 ** 40 + 9, sweeps=1)
    on = _device(case, 65, seed=2 ** 40 + 9, sweeps=3, state=first["draw_state"], first_sweep=2)
    assert torch.equal(on["draw_state"], a["draw_state"]) and torch.equal(_bits(on["filtered"]), _bits(a["filtered"]))
    traced = _device(case, 65, seed=2 ** 40 + 9, sweeps=3, trace=True)          # sweep by sweep: the same draws, and the trace
    assert torch.equal(traced["draw_state"], a["draw_state"]) and traced["log_score_trace"].shape == (4, 65) and traced["change_share"].shape == (3,)
    x = a["draw_state"].cpu().numpy()
    terms = np.concatenate([score[np.arange(12)[None, :], x], -(g[None, :] * d2[np.arange(eu.size)[None, :], x[:, eu], x[:, ev]])], axis=1)
    assert np.all(np.abs(traced["log_score_trace"][3].cpu().numpy() - terms.sum(axis=1)) <= terms.shape[1] * U * np.abs(terms).sum(axis=1))
    share = traced["change_share"].cpu().numpy()
    assert np.all(share > 0.0) and np.all(share <= 1.0)
    none = sections.graph_draw(torch.zeros((0, 5, 5), dtype=torch.float64, device=dev), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                               np.zeros(0, dtype=np.int32), [0], 3)
    assert none["draw_state"].shape == (3, 0) and none["filtered"].shape == (3, 0, 5)


def test_the_devices_own_draws_reach_the_exact_joint_of_the_ladder():
    eu, ev, g, d2, n_used, score, ptr = ladder_case()
    got = _numpy(_device((eu, ev, g, d2, n_used, score, ptr), R_STAT, seed=LADDER_SEED, sweeps=LADDER_SWEEPS))
    check_ladder(got["draw_state"], "device, ladder, %d sweeps" % LADDER_SWEEPS)


def test_the_c_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    S, E, n, L, R = 4, 3, 3, 2, 5                                              # two lines of two, a step each and one cross edge
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)      # noqa: E731
    a = dict(S=S, E=E, n=n, L=L, ptr=torch.tensor([0, 2, 4], dtype=torch.int64, device=dev), eu=i32([0, 0, 2]), ev=i32([1, 2, 3]), nu=i32([3, 3, 3, 3]),
             score=torch.zeros((S, n), dtype=torch.float64, device=dev), g=torch.ones(E, dtype=torch.float64, device=dev),
             d2=torch.zeros((E, n, n), dtype=torch.float64, device=dev), ready=0, K=f64(E, n, n), step=i32([0, -1, 2, -1]), cptr=i32([0, 1, 1, 2, 2]),
             cedge=i32([3, 2]), ncol=2, colptr=i32([0, 1, 2]), colline=i32([0, 1]), key=None, seed=1, R=R, first=0, t0=0, t1=2, w=f64(S, n), fl=f64(R, S, n),
             sc=f64(R, S), ds=torch.full((R, S), 7, dtype=torch.int32, device=dev))
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                    # noqa: E731

    def call(**kw):
        b = dict(a, **kw)
        return lib.gbp_section_graph_draw(*[p(b[name]) for name in ("S", "E", "n", "L", "ptr", "eu", "ev", "nu", "score", "g", "d2", "ready", "K", "step", "cptr", "cedge",
                                                                  "ncol", "colptr", "colline", "key", "seed", "R", "first", "t0", "t1", "w", "fl", "sc", "ds")], st)

    for kw in (dict(S=-1), dict(E=-1), dict(E=2 ** 30), dict(n=0), dict(n=257), dict(L=-1), dict(L=0), dict(R=0), dict(R=65537), dict(first=-1), dict(first=65536 - R + 1),
               dict(t0=-1), dict(t0=3), dict(t1=65536), dict(S=1), dict(ncol=0), dict(ncol=3), dict(L=2 ** 20, R=65536), dict(ptr=None), dict(nu=None), dict(score=None), dict(step=None), dict(cptr=None), dict(colptr=None), dict(colline=None),
               dict(w=None), dict(fl=None), dict(sc=None), dict(ds=None), dict(eu=None), dict(ev=None), dict(K=None), dict(cedge=None), dict(g=None), dict(d2=None)):
        assert call(**kw) != 0 and b"gbp_section_graph_draw" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((a[name] == 7).all()) for name in ("K", "w", "fl", "sc", "ds"))      # nothing was written
    assert call(S=0, E=0, L=0, ptr=None, nu=None) == 0                         # no sounding: OK without a launch
    torch.cuda.synchronize()
    assert bool((a["ds"] == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    first = a["ds"].clone()
    assert bool((first >= 0).all()) and bool((first < n).all()) and bool((a["sc"] != 7.0).all()) and bool((a["K"] == 1.0).all())
    assert call(ready=1, g=None, d2=None) == 0                                 # K is there: g and d2 are not read
    torch.cuda.synchronize()
    assert torch.equal(a["ds"], first)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

def test_the_planted_lines_with_draws():
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    ens = _to_device(k, edges, sigma)
    S, n = k.shape
    R = 64
    kw = dict(ptr=ptr, max_models=n, max_distance=1.5 * SPACING)
    plain = sections.spatial(ens, x, y, Z1_LINES, **kw)
    out = sections.spatial(ens, x, y, Z1_LINES, draws=R, seed=2, **kw)
    new = {"draw_state", "draw_slot", "draw_log_score", "draw_share", "draw_change_share"}
    assert set(out) == set(plain) | new and not new & set(plain)
    for name in plain:                                                         # draws change no other output
        assert torch.equal(_bits(out[name]), _bits(plain[name])), name
    o = _numpy(out)
    assert o["draw_state"].shape == (R, S) and o["draw_state"].dtype == np.int32 and o["draw_slot"].dtype == np.int32 and o["draw_log_score"].shape == (R,)
    assert o["draw_share"].shape == (S, n) and o["draw_change_share"].shape == (8,)
    assert np.array_equal(o["draw_slot"], o["rows"][np.arange(S)[None, :], o["draw_state"]])
    depth_edges = np.arange(0.0, Z1_LINES + 1.0, 5.0)
    models = _numpy(sections.draw_models(ens, out["draw_slot"], depth_edges=depth_edges))
    assert models["raster"].shape == (R, S, depth_edges.size - 1) and np.all(np.isfinite(models["raster"]))
    assert np.array_equal(models["k"], k[np.arange(S)[None, :], o["draw_slot"]]) and np.array_equal(models["edges"], edges[np.arange(S)[None, :], o["draw_slot"]])
    assert float(np.abs(o["draw_share"].sum(axis=1) - 1.0).max()) <= n * U
    counts = np.stack([np.bincount(o["draw_state"][:, s], minlength=n) for s in range(S)])
    assert np.array_equal(o["draw_share"], counts / R)
    # the rule on the device's own distances; the key of a sounding is its index
    eu, ev, g, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * SPACING)
    d2 = sections.edge_distance(ens, out["rows"], eu, ev, 0.0, Z1_LINES).cpu().numpy()
    ref = sections.graph_draw_reference(eu, ev, g, d2, o["n_used"], ptr, R, seed=2)
    keep = (ref["margin"] >= CLOSE).all(axis=1)
    print("planted lines: %d of %d realisations left out" % (int((~keep).sum()), R))
    assert (~keep).sum() <= 0.01 * R and np.array_equal(o["draw_state"][keep], ref["draw_state"][keep])
    xs = o["draw_state"]
    terms = -(g[None, :] * d2[np.arange(eu.size)[None, :], xs[:, eu], xs[:, ev]])
    assert np.all(np.abs(o["draw_log_score"] - terms.sum(axis=1)) <= eu.size * U * np.abs(terms).sum(axis=1))
    # what the coupling is for: alone the centre of the middle line sits on its decoy, with its neighbours on the true family
    alone = _numpy(sections.spatial(ens, x, y, Z1_LINES, draws=R, seed=2, draw_sweeps=0, **kw))
    assert alone["draw_change_share"].shape == (0,)
    print("the true family's share at the centre of the middle line: alone %.3f, across lines %.3f" % (true_share(alone["draw_state"]), true_share(xs)))
    assert true_share(xs) > true_share(alone["draw_state"])
    assert true_share(xs) > 0.5
    # a sounding without models is left out of the graph and cuts its line; its key stays its index in the survey
    kk = ens.k.clone()
    kk[9] = 0
    cut = _numpy(sections.spatial(ens._replace(k=kk), x, y, Z1_LINES, draws=R, seed=2, **kw))
    at = np.arange(S) != 9
    assert np.all(cut["draw_state"][:, 9] == -1) and np.all(cut["draw_slot"][:, 9] == -1) and np.isnan(cut["draw_share"][9]).all()
    assert np.all(cut["draw_state"][:, at] >= 0) and np.all(cut["draw_state"][:, at] < n) and not np.isnan(cut["draw_share"][at]).any()
    keep9 = np.flatnonzero(at)
    local = np.cumsum(at) - 1
    eu9, ev9, g9, _ = sections.neighbours(x, y, ptr, cut["n_used"], max_distance=1.5 * SPACING)
    d29 = sections.edge_distance(ens._replace(k=kk), torch.as_tensor(cut["rows"]).to(_dev()), eu9, ev9, 0.0, Z1_LINES).cpu().numpy()
    ref9 = sections.graph_draw_reference(local[eu9], local[ev9], g9, d29, cut["n_used"][at], [0, 8, 9, 15, 23], R, seed=2, row_key=keep9)
    keep = (ref9["margin"] >= CLOSE).all(axis=1)
    assert (~keep).sum() <= 0.01 * R and np.array_equal(cut["draw_state"][keep][:, at], ref9["draw_state"][keep])


def test_from_survey_and_the_command_line_with_draws(tmp_path):
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    survey = dict(ensemble_k=k, ensemble_edges=edges, ensemble_sigma=sigma, line=np.repeat([10, 20, 30], S_LINES), x=x, y=y, fiducial=np.arange(k.shape[0]))
    direct = _numpy(sections.spatial_from_survey(survey, Z1_LINES, max_models=16, max_distance=150.0, sweeps=12, draws=4, seed=3, draw_sweeps=5))
    both = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, spatial=dict(max_models=16, max_distance=150.0, sweeps=12, draws=4, seed=3, draw_sweeps=5)))
    assert direct["draw_state"].shape == (4, 24) and direct["draw_change_share"].shape == (5,) and direct["draw_log_score"].shape == (4,)
    for name in direct:
        if name not in ("line", "fiducial", "x", "y"):
            assert np.array_equal(both["spatial_" + name], direct[name], equal_nan=True), name
    assert "draw_state" not in both                                            # the lines' own draws were not asked for
    path = str(tmp_path / "survey.npz")
    np.savez(path, **survey)
    written = sections.main([path, "--depth", "120", "--spatial", "150", "--sweeps", "12", "--max-models", "16", "--spatial-draws", "4", "--seed", "3", "--draw-sweeps", "5"])
    f = sections.load(written)
    assert written == str(tmp_path / "survey.spatial.npz") and set(f) == set(direct)
    assert all(np.array_equal(f[name], direct[name], equal_nan=True) for name in direct)
    other = _numpy(sections.spatial_from_survey(survey, Z1_LINES, max_models=16, max_distance=150.0, sweeps=12, draws=4, seed=4, draw_sweeps=5))
    assert not np.array_equal(other["draw_state"], direct["draw_state"]) and np.array_equal(other["weight"], direct["weight"], equal_nan=True)
    assert "draw_state" not in sections.load(sections.main([path, "--depth", "120", "--spatial", "150", "--max-models", "16"]))
