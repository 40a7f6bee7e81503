"""The host side of the sections of sampled models (geobipy_amd/sections.py): ``track_reference`` against the
enumeration of every path, ``cross_distance_reference`` against the stacked ``families.distance_reference``, ``partners`` / ``pieces`` /
``steps`` against their definitions, every refusal that comes before the library loads, and the planted line on the rules alone."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, ensembles, families, sections

# ---- the chain against the enumeration of every path ----------------------------------------------------------------------------------


def _enumerate(score, g, d2, n_used, dtype):
    """One sequence by brute force: (the path the rule must pick, its score, the marginals [N, n]).  The score of a path is evaluated as
    the rule evaluates it, V <- score[r + 1, j] + (V - g[r] * d2[r, i, j]); among the paths of maximal score the rule's tie order picks
    the one with the lowest last state, then the lowest state before it, and so on.  The marginals are the sums of the path weights."""
    ft = np.dtype(dtype).type
    N, n = score.shape
    sc, gg, dd = score.astype(ft), g.astype(ft), d2.astype(ft)
    best, best_path = None, None
    weight = np.zeros((N, n), dtype=np.longdouble)
    for path in itertools.product(*[range(int(m)) for m in n_used]):
        v = sc[0, path[0]]
        lw = np.longdouble(score[0, path[0]])
        for r in range(N - 1):
            v = sc[r + 1, path[r + 1]] + (v - gg[r] * dd[r, path[r], path[r + 1]])
            lw = lw + np.longdouble(score[r + 1, path[r + 1]]) - np.longdouble(g[r]) * np.longdouble(d2[r, path[r], path[r + 1]])
        if best is None or v > best or (v == best and path[::-1] < best_path[::-1]):
            best, best_path = v, path
        for r in range(N):
            weight[r, path[r]] += np.exp(lw)
    return np.array(best_path), best, weight / weight.sum(axis=1, keepdims=True)


def _random_chain(rng, lengths, n, exact=False):
    total = int(np.sum(lengths))
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    n_used = rng.integers(1, n + 1, total)
    n_used[0], n_used[-1] = 1, n
    if exact:                                                                  # every operation exact: ties are ties
        score, g, d2 = rng.integers(0, 3, (total, n)).astype(np.float64), np.ones(total), rng.integers(0, 9, (total, n, n)) / 8.0
    else:
        score, g, d2 = rng.normal(0.0, 1.0, (total, n)), rng.uniform(0.5, 3.0, total), rng.uniform(0.0, 2.0, (total, n, n))
    for r in range(total):                                                     # nothing outside the prefixes is read
        d2[r, n_used[r]:, :] = np.nan
        if r + 1 < total:
            d2[r, :, n_used[r + 1]:] = np.nan
    return ptr, score, g, d2, n_used


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("exact", [False, True])
def test_track_reference_against_every_path(dtype, exact):
    rng = np.random.default_rng(11 + exact)
    for n, lengths in ((1, (1, 3)), (2, (5, 1, 2)), (3, (4, 5)), (4, (5, 3, 1))):
        ptr, score, g, d2, n_used = _random_chain(rng, lengths, n, exact)
        got = sections.track_reference(ptr, score, g, d2, n_used, dtype=dtype)
        assert got["state"].dtype == np.int32 and got["marginal"].shape == (ptr[-1], n)
        for l, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
            cut = d2[a:b].copy()
            path, top, gamma = _enumerate(score[a:b], g[a:b], np.nan_to_num(cut), n_used[a:b], dtype)
            assert np.array_equal(got["state"][a:b], path), (n, l, exact)
            assert got["log_score"][l] == top, (n, l)
            assert np.all(got["state"][a:b] < n_used[a:b])
            assert float(np.abs(got["marginal"][a:b] - gamma).max()) <= 1e-13, (n, l)
            for r in range(a, b):
                assert np.all(got["marginal"][r, n_used[r]:] == 0.0)
        assert np.allclose(got["marginal"].sum(axis=1).astype(np.float64), 1.0, rtol=0, atol=1e-13)
        only = sections.track_reference(ptr, score, g, d2, n_used, marginals=False, dtype=dtype)
        assert set(only) == {"state", "log_score"} and np.array_equal(only["state"], got["state"])
    # score=None is zeros
    ptr, score, g, d2, n_used = _random_chain(rng, (4,), 3)
    a, b = sections.track_reference(ptr, None, g, d2, n_used), sections.track_reference(ptr, np.zeros((4, 3)), g, d2, n_used)
    assert all(np.array_equal(a[name], b[name]) for name in a)
    # the partition function is the sum over the paths
    w = sum(np.exp(-sum(g[r] * d2[r, p[r], p[r + 1]] for r in range(3))) for p in itertools.product(*[range(int(m)) for m in n_used]))
    assert abs(a["log_partition"][0] - np.log(w)) <= 1e-13 and abs(np.log(a["scale"]).sum() - a["log_partition"][0]) <= 1e-14


def test_a_nan_candidate_never_wins_and_underflow_gives_nan_marginals():
    ptr, g, n_used = np.array([0, 3]), np.ones(3), np.array([2, 2, 2])
    d2 = np.array([[[np.nan, 1.0], [2.0, np.nan]], [[0.5, 4.0], [np.nan, np.nan]], [[0.0, 0.0], [0.0, 0.0]]])
    got = sections.track_reference(ptr, None, g, d2, n_used, marginals=False)
    assert got["state"].tolist() == [1, 0, 0] and got["log_score"][0] == -2.5      # 1 -> 0 costs 2.0, 0 -> 0 costs 0.5; every NaN is passed over
    d2 = np.full((3, 2, 2), 1.0e4)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = sections.track_reference(ptr, None, g, d2, n_used)
    assert np.isnan(out["marginal"]).all() and out["state"].tolist() == [0, 0, 0]


# ---- the cross distance -------------------------------------------------------------------------------------------------------------

def _three_soundings(seed=3, ns=6, K=4):
    rng = np.random.default_rng(seed)
    k = rng.integers(1, K + 1, (3, ns)).astype(np.int32)
    k[1, 2] = 0                                                                # an empty slot
    edges, sigma = np.full((3, ns, K), np.inf), np.full((3, ns, K), np.nan)
    for s in range(3):
        for t in range(ns):
            edges[s, t, :max(k[s, t] - 1, 0)] = np.sort(rng.uniform(0.0, 60.0, max(k[s, t] - 1, 0)))
            sigma[s, t, :k[s, t]] = 10.0 ** rng.uniform(-3.0, 0.0, k[s, t])
    k[2, 0], edges[2, 0], sigma[2, 0] = k[0, 1], edges[0, 1], sigma[0, 1]      # sounding 2 holds a copy of a model of sounding 0
    rows = np.array([[1, 0, 5, -1, 3], [2, 4, 6, 1, 0], [0, 3, 3, 2, 2 ** 30]], dtype=np.int32)
    return k, edges, sigma, rows


@pytest.mark.parametrize("measure,z0", [("linear", 0.0), ("log", 2.0)])
def test_cross_distance_reference_is_the_stacked_block(measure, z0):
    k, edges, sigma, rows = _three_soundings()
    ns, n = k.shape[1], rows.shape[1]
    partner = np.array([2, 0, -1], dtype=np.int32)
    for squared in (True, False):
        got = sections.cross_distance_reference(k, edges, sigma, rows, partner, z0, 50.0, measure=measure, squared=squared)
        assert got.shape == (3, n, n) and np.isnan(got[2]).all()                # partner -1: a slab of NaN
        for s, p in ((0, 2), (1, 0)):
            valid = lambda r: np.where((r >= 0) & (r < ns), r, -1)             # noqa: E731
            stacked = np.concatenate([valid(rows[s]), np.where(valid(rows[p]) >= 0, valid(rows[p]) + ns, -1)])
            want = families.distance_reference(np.concatenate([k[s], k[p]]), np.concatenate([edges[s], edges[p]]), np.concatenate([sigma[s], sigma[p]]),
                                               stacked, z0, 50.0, measure=measure, squared=squared)[:n, n:]
            assert np.array_equal(got[s], want, equal_nan=True)
        assert np.isnan(got[0][3]).all() and np.isnan(got[0][:, 4]).all()      # row -1 of sounding 0; the row past the end of sounding 2
        assert np.isnan(got[1][0]).all() and np.isnan(got[1][2]).all()         # the empty slot and the row past the end of sounding 1
        assert got[0][0, 0] == 0.0 and np.isfinite(got[0][0, 1]) and got[0][0, 1] > 0      # the copy: 0.0 by arithmetic, no diagonal
        both = sections.cross_distance_reference(k, edges, sigma, rows, [1, 0, 7], z0, 50.0, measure=measure, squared=squared)
        assert np.array_equal(both[0], both[1].T, equal_nan=True) and np.isnan(both[2]).all()      # the pair the other way round
    ld = sections.cross_distance_reference(k, edges, sigma, rows, partner, z0, 50.0, measure=measure, dtype=np.longdouble)
    assert ld.dtype == np.longdouble and np.allclose(ld.astype(np.float64), sections.cross_distance_reference(k, edges, sigma, rows, partner, z0, 50.0, measure=measure),
                                                     rtol=1e-13, atol=0, equal_nan=True)
    with pytest.raises(ValueError, match="cross_distance_reference"):
        sections.cross_distance_reference(k, edges, sigma, rows, partner[:2], z0, 50.0)


# ---- partners, pieces, steps ---------------------------------------------------------------------------------------------------------

def test_partners_cut_at_empty_soundings():
    ptr = np.array([0, 4, 5, 9])
    n_used = np.array([3, 3, 3, 3, 2, 4, 0, 4, 4], dtype=np.int32)
    assert sections.partners(ptr, n_used).tolist() == [1, 2, 3, -1, -1, -1, -1, 8, -1]
    assert sections.partners(ptr, n_used).dtype == np.int32
    assert sections.partners(None, np.array([1, 1, 0, 0, 1])).tolist() == [1, -1, -1, -1, -1]
    assert sections.partners(None, torch.tensor([2, 2])).tolist() == [1, -1] and sections.partners(None, np.zeros(0, dtype=np.int32)).size == 0
    keep, piece_ptr, owner = sections.pieces(ptr, n_used)
    assert keep.tolist() == [0, 1, 2, 3, 4, 5, 7, 8] and piece_ptr.tolist() == [0, 4, 5, 6, 8] and owner.tolist() == [0, 1, 2, 2]
    keep, piece_ptr, owner = sections.pieces(None, np.array([0, 0]))
    assert keep.size == 0 and piece_ptr.tolist() == [0] and owner.size == 0
    assert sections.line_ptr([3, 3, 1, 1, 1, 3]).tolist() == [0, 2, 5, 6] and sections.line_ptr([]).tolist() == [0]


def test_steps_against_the_formula():
    x, y = np.array([0.0, 30.0, 30.0, 30.5, 100.0]), np.array([0.0, 40.0, 40.0, 40.0, 40.0])
    g = sections.steps(x, y)
    dx = np.array([50.0, 0.0, 0.5, 69.5, 0.0])
    assert np.array_equal(g, 100.0 / (2.0 * 0.1 * 0.1 * np.maximum(dx, 1.0)))
    g = sections.steps(x, y, tau=0.25, length=40.0, min_distance=2.0, ptr=[0, 1, 5])
    dx[0] = 0.0                                                                # the last sounding of the first sequence
    assert np.array_equal(g, 40.0 / (2.0 * 0.25 * 0.25 * np.maximum(dx, 2.0)))
    assert sections.steps([], []).size == 0
    for kw, match in ((dict(tau=0.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(length=-1.0), "length"), (dict(min_distance=0.0), "min_distance"),
                      (dict(tau=True), "tau")):
        with pytest.raises(ValueError, match=match):
            sections.steps(x, y, **kw)
    with pytest.raises(ValueError, match="one entry per sounding"):
        sections.steps(x, y[:3])
    with pytest.raises(ValueError, match="finite"):
        sections.steps(x, np.where(y > 0, np.inf, y))
    with pytest.raises(ValueError, match="ptr must start at 0"):
        sections.steps(x, y, ptr=[0, 2, 4])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _host_ensemble(S=2, ns=8, K=4):
    k = torch.ones((S, ns), dtype=torch.int32)
    e = torch.full((S, ns, K), float("inf"), dtype=torch.float64)
    s = torch.ones((S, ns, K), dtype=torch.float64)
    return ensembles.Ensemble(k, e, s, torch.zeros((S, ns), dtype=torch.float64), (k > 0).sum(dim=1), 1, torch.zeros(S, dtype=torch.float64))


def test_refusals_come_before_the_library():
    for bad, match in ((np.zeros((2, 2)), "vector"), (np.array([0.0, 3.0]), "vector"), ([1, 3], "start at 0"), ([0, 2], "end at"), ([0, 1, 1, 3], "at least one")):
        with pytest.raises(ValueError, match=match):
            sections.check_ptr(bad, 3)
    ens = _host_ensemble()
    rows, partner = torch.zeros((2, 5), dtype=torch.int32), np.array([1, -1], dtype=np.int32)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.cross_distance(ens, rows.numpy(), partner, 0.0, 10.0)
    for bad in (dict(k=ens.k[:, :3]), dict(edges=ens.edges[:, :, :2]), dict(sigma=ens.sigma[0])):
        with pytest.raises(ValueError, match="ensemble"):
            sections.cross_distance(ens._replace(**bad), rows, partner, 0.0, 10.0)
    for bad_rows in (rows[0], rows[:1], torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 4097), dtype=torch.int32)):
        with pytest.raises(ValueError, match="rows"):
            sections.cross_distance(ens, bad_rows, partner, 0.0, 10.0)
    with pytest.raises(TypeError):
        sections.cross_distance(ens, rows.long(), partner, 0.0, 10.0)
    for bad_partner in (partner[:1], np.array([1.0, -1.0]), np.zeros((2, 1), dtype=np.int32)):
        with pytest.raises(ValueError, match="partner"):
            sections.cross_distance(ens, rows, bad_partner, 0.0, 10.0)
    for kw in (dict(z0=-1.0), dict(z1=0.0), dict(measure="cubic"), dict(measure="log"), dict(block=0)):
        with pytest.raises(ValueError):
            sections.cross_distance(ens, rows, partner, **dict(dict(z0=0.0, z1=10.0), **kw))
    with pytest.raises(_lib.NativeLibraryError, match="gbp_ensemble_cross_distance"):
        sections.cross_distance(ens, rows, partner, 0.0, 10.0)

    d2, g, ptr, n_used = torch.zeros((3, 4, 4), dtype=torch.float64), np.ones(3), [0, 3], np.array([4, 1, 2])
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.track(d2.numpy(), g, ptr, n_used)
    for track in (sections.track, lambda d2_, g_, p_, nu_, score=None: sections.track_reference(p_, score, g_, d2_, nu_)):
        for bad, match in (((d2[0], g, ptr, n_used), "d2"), ((d2[:, :3], g, ptr, n_used), "d2"), ((d2, g[:2], ptr, n_used), "g must"),
                           ((d2, g, [0, 2], n_used), "ptr"), ((d2, g, ptr, n_used[:2]), "n_used"), ((d2, g, ptr, np.array([4, 0, 2])), "1 .. n"),
                           ((d2, g, ptr, np.array([4, 5, 2])), "1 .. n"), ((d2, g, ptr, np.array([4.0, 1.0, 2.0])), "n_used")):
            with pytest.raises(ValueError, match=match):
                track(*bad)
        with pytest.raises(ValueError, match="score"):
            track(d2, g, ptr, n_used, score=torch.zeros((3, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="n <= 1024"):
        sections.track(torch.zeros((3, 1025, 1025), dtype=torch.float64)[:0], g[:0], [0], n_used[:0])
    with pytest.raises(TypeError):
        sections.track(d2.float(), g, ptr, n_used)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_track"):
        sections.track(d2, g, ptr, n_used)

    x = y = np.zeros(2)
    for kw in (dict(z1=0.0), dict(measure="log"), dict(chains=3), dict(max_models=0), dict(max_models=1025), dict(tau=0.0), dict(length=0.0),
               dict(min_distance=-1.0), dict(ptr=[0, 1]), dict(budget_bytes=0), dict(score=torch.zeros((2, 5), dtype=torch.float64))):
        with pytest.raises(ValueError):
            sections.sections(ens, x, y, **dict(dict(z1=10.0), **kw))
    with pytest.raises(ValueError, match="one entry per sounding"):
        sections.sections(ens, np.zeros(3), np.zeros(3), 10.0)
    with pytest.raises(ValueError, match="max_models.*budget_bytes"):                       # 2 soundings x 8 x 8 doubles do not fit 500 bytes
        sections.sections(ens, x, y, 10.0, budget_bytes=500)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.sections(ens._replace(k=ens.k.numpy()), x, y, 10.0)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.sections(ens, x, y, 10.0)
    with pytest.raises(ValueError, match="ensemble_k"):
        sections.from_survey(dict(line=np.zeros(2), x=x, y=y), 10.0)
    with pytest.raises(ValueError, match="ptr is not taken"):
        sections.from_survey(dict(ensemble_k=ens.k.numpy(), ensemble_edges=ens.edges.numpy(), ensemble_sigma=ens.sigma.numpy(), line=np.zeros(2), x=x, y=y),
                             10.0, ptr=[0, 2])


def test_the_command_line_refuses_before_any_device_work(capsys):
    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--from", "2", "--measure", "log", "--tau", "0.2", "--length", "50", "--max-models", "64",
                                    "--chains", "2", "--no-marginals"])
    assert path == "run.npz" and kw == dict(z1=150.0, z0=2.0, measure="log", tau=0.2, length=50.0, max_models=64, chains=2, marginals=False,
                                            device="cuda:0")
    assert sections.output_path("a/run.npz") == "a/run.sections.npz"
    for argv in (["run.npz"], ["run.npz", "--depth", "0"], ["run.npz", "--depth", "10", "--measure", "log"], ["run.npz", "--depth", "10", "--tau", "0"],
                 ["run.npz", "--depth", "10", "--max-models", "2000"], ["run.npz", "--depth", "10", "--chains", "0"]):
        with pytest.raises(SystemExit):
            sections.parse_args(argv)
    capsys.readouterr()


def test_signatures_declare_both_entries():
    assert len(_lib.SIGNATURES["gbp_ensemble_cross_distance"][1]) == 16 and len(_lib.SIGNATURES["gbp_section_track"][1]) == 15


# ---- the planted line ---------------------------------------------------------------------------------------------------------------

S_LINE, N_LINE, Z1_LINE = 40, 16, 120.0


def planted_line():
    """40 soundings, 25 m apart, of 16 three-layer models (K = 4).  The first interface of the true family lies at 30 + 10 sin(s / 6) m,
    +- 1 m of normal jitter; in about 30 % of the soundings 10 of the 16 models belong to a decoy family whose first interface is 15 m
    above or below the true one, the sign drawn per sounding.  Returns (k [S, n], edges, sigma [S, n, K], x, y, truth [S])."""
    rng = np.random.default_rng(7)
    S, n, K = S_LINE, N_LINE, 4
    truth = 30.0 + 10.0 * np.sin(np.arange(S) / 6.0)
    k = np.full((S, n), 3, dtype=np.int32)
    edges, sigma = np.full((S, n, K), np.inf), np.full((S, n, K), np.nan)
    decoy = rng.uniform(size=S) < 0.3
    sign = rng.choice([-15.0, 15.0], S)
    for s in range(S):
        top = truth[s] + rng.normal(0.0, 1.0, n)
        if decoy[s]:
            top[:10] += sign[s]
        edges[s, :, 0] = top
        edges[s, :, 1] = 80.0 + rng.normal(0.0, 1.0, n)
        sigma[s, :, :3] = 10.0 ** (np.array([-2.0, -0.5, -1.5]) + rng.normal(0.0, 0.05, (n, 3)))
    return k, edges, sigma, 25.0 * np.arange(S), np.zeros(S), truth


def check_planted_line(state_of, k, edges, sigma, x, y, truth):
    """The assertions of the planted line, given ``state_of(g)`` -> the path for the steps g: every chosen model's first interface lies
    within 4 m of the planted one (4 sigma of the 1 m jitter), the path is the same for tau = 0.05 and 0.4, and -- a property of the
    inputs, so that the test says something -- the per-sounding medoid is more than 10 m off in at least 20 % of the soundings."""
    S, n = k.shape
    rows = np.arange(n)
    off = np.zeros(S)
    for s in range(S):
        D = families.distance_reference(k[s], edges[s], sigma[s], rows, 0.0, Z1_LINE)
        off[s] = abs(edges[s, int(np.argmin(np.cumsum(D, axis=0)[-1])), 0] - truth[s])
    print("per-sounding medoid: more than 10 m off in %.0f %% of the soundings" % (100.0 * np.mean(off > 10.0)))
    assert np.mean(off > 10.0) >= 0.2
    paths = {tau: state_of(sections.steps(x, y, tau=tau)) for tau in (0.05, 0.1, 0.4)}
    chosen = edges[np.arange(S), paths[0.1], 0]
    print("path: at most %.2f m from the planted interface" % np.abs(chosen - truth).max())
    assert np.all(np.abs(chosen - truth) <= 4.0)
    assert np.array_equal(paths[0.05], paths[0.4]) and np.array_equal(paths[0.05], paths[0.1])


def test_the_planted_line_on_the_rules_alone():
    k, edges, sigma, x, y, truth = planted_line()
    S, n = k.shape
    rows = np.tile(np.arange(n, dtype=np.int32), (S, 1))
    n_used = np.full(S, n, dtype=np.int32)
    partner = sections.partners(None, n_used)
    assert partner.tolist() == list(range(1, S)) + [-1]
    d2 = sections.cross_distance_reference(k, edges, sigma, rows, partner, 0.0, Z1_LINE)
    assert np.isnan(d2[-1]).all() and np.isfinite(d2[:-1]).all()
    check_planted_line(lambda g: sections.track_reference([0, S], None, g, d2, n_used, marginals=False)["state"], k, edges, sigma, x, y, truth)
    out = sections.track_reference([0, S], None, sections.steps(x, y), d2, n_used)
    n_eff = 1.0 / (out["marginal"] ** 2).sum(axis=1)
    assert np.all(n_eff >= 1.0 - 1e-12) and np.all(n_eff <= n + 1e-9)
    two_family = np.abs(edges[:, :, 0] - truth[:, None]).max(axis=1) > 10.0       # the soundings with a decoy: its ten models lose their weight
    assert two_family.any() and np.all(out["marginal"][two_family, :10].sum(axis=1) < 1e-3)
