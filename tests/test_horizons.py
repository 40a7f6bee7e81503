"""Horizon tracking, the host side (geobipy_amd.horizons): the numpy rule against brute-force enumeration of every
path, the tie order, the degenerate cases, the evidence-to-score rule, the window-by-slicing identity, the steps, the argument checks
of Python, the command line and the C entry, and a planted dipping horizon under terrain that the per-sounding argmax cannot find."""
import ctypes
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import horizons as hz


def _problem(rng, N, S, absent):
    score = rng.normal(0.0, 2.0, (N, S))
    ab = rng.normal(0.0, 2.0, N) if absent else None
    g = rng.uniform(0.2, 1.5, N)
    d = rng.normal(0.0, 1.0, N)
    return score, ab, g, d


def _brute(score, ab, g, d, dz, switch):
    """Every path of the chain: the best one with its score (summed in the order of the recursion) and the marginals / evidence."""
    N, S = score.shape
    SA = S + (ab is not None)
    full = score if ab is None else np.concatenate([score, ab[:, None]], axis=1)

    def cost(n, a, b):
        if a < S and b < S:
            return g[n] * abs(d[n] - float(b - a) * dz)
        return 0.0 if a == b else switch

    best, best_path = -np.inf, None
    weight = {}
    for path in itertools.product(range(SA), repeat=N):
        v = full[0, path[0]]
        lw = full[0, path[0]]
        for n in range(N - 1):
            t = cost(n, path[n], path[n + 1])
            v = full[n + 1, path[n + 1]] + (v - t)
            lw += full[n + 1, path[n + 1]] - t
        weight[path] = np.exp(lw)
        if v > best:
            best, best_path = v, path
    Z = sum(weight.values())
    gamma = np.zeros((N, SA))
    for path, wt in weight.items():
        for n, c in enumerate(path):
            gamma[n, c] += wt / Z
    return np.array(best_path), best, gamma, np.log(Z)


@pytest.mark.parametrize("absent", [False, True])
def test_the_rule_against_every_path(absent):
    rng = np.random.default_rng(11 + absent)
    N, S, dz, switch = 4, 3, 0.5, 1.3
    for _ in range(5):
        score, ab, g, d = _problem(rng, N, S, absent)
        r = hz.track_reference([0, N], score, ab, g, d, dz, switch)
        path, best, gamma, logZ = _brute(score, ab, g, d, dz, switch)
        assert np.array_equal(r["cell"], path)
        assert r["log_score"][0] - best == 0.0
        err = np.abs(r["marginal"] - gamma).max()
        print("max |marginal - enumeration| = %.3g, |log_partition - ln Z| = %.3g" % (err, abs(r["log_partition"][0] - logZ)))
        assert err <= 1e-14 and abs(r["log_partition"][0] - logZ) <= 1e-14
        assert np.allclose(r["marginal"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
        assert abs(np.log(r["scale"]).sum() - r["log_partition"][0]) <= 1e-14


def test_several_sequences_are_independent():
    rng = np.random.default_rng(3)
    parts = [_problem(rng, n, 5, True) for n in (1, 2, 7)]
    cat = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    r = hz.track_reference([0, 1, 3, 10], cat[0], cat[1], cat[2], cat[3], 0.5, 2.0)
    r0 = 0
    for l, p in enumerate(parts):
        one = hz.track_reference([0, len(p[2])], p[0], p[1], p[2], p[3], 0.5, 2.0)
        n = len(p[2])
        assert np.array_equal(one["cell"], r["cell"][r0:r0 + n]) and one["log_score"][0] == r["log_score"][l]
        assert np.array_equal(one["marginal"], r["marginal"][r0:r0 + n]) and one["log_partition"][0] == r["log_partition"][l]
        r0 += n


def test_tie_order_lowest_cell_first_and_a_cell_before_absent():
    z = np.zeros
    # every path scores the same: the lowest cell everywhere, never the absent state (switch 0: entering it is free, and still a tie)
    r = hz.track_reference([0, 3], z((3, 3)), None, np.ones(3), z(3), 1.0, 0.0, marginals=False)
    assert np.array_equal(r["cell"], [0, 0, 0]) and r["log_score"][0] == 0.0
    r = hz.track_reference([0, 3], z((3, 3)), z(3), z(3), z(3), 1.0, 0.0, marginals=False)
    assert np.array_equal(r["cell"], [0, 0, 0]) and r["log_score"][0] == 0.0
    # cell 1 under the second sounding is reached from cells 0 and 2 at the same price: the pointer goes to the lower one
    score = np.array([[5.0, 0.0, 5.0], [-10.0, 0.0, -10.0]])
    r = hz.track_reference([0, 2], score, None, np.ones(2), z(2), 1.0, 0.0, marginals=False)
    assert np.array_equal(r["cell"], [0, 1]) and r["log_score"][0] == 4.0
    # the absent state wins only when strictly better, at the end of the path and as a predecessor
    r = hz.track_reference([0, 2], z((2, 2)), np.array([-1.0, 1.0]), np.ones(2), z(2), 1.0, 1.0, marginals=False)
    assert np.array_equal(r["cell"], [0, 0]) and r["log_score"][0] == 0.0          # absent ends at 1 - 1 = 0: a tie, the cell stays
    r = hz.track_reference([0, 2], z((2, 2)), np.array([-1.0, 2.0]), np.ones(2), z(2), 1.0, 1.0, marginals=False)
    assert np.array_equal(r["cell"], [0, 2]) and r["log_score"][0] == 1.0          # into absent from cell 0 (0 - 1) or absent (-1): the cell
    r = hz.track_reference([0, 2], z((2, 2)), np.array([0.0, 1.5]), np.ones(2), z(2), 1.0, 1.0, marginals=False)
    assert np.array_equal(r["cell"], [2, 2]) and r["log_score"][0] == 1.5          # 0 + 1.5 from absent (free) beats 0.5 through a switch


def test_one_sounding_has_no_step():
    score = np.array([[0.1, 1.2, -0.3]])
    r = hz.track_reference([0, 1], score, None, [1.0], [0.0], 0.5, 1.0)
    assert r["cell"][0] == 1 and r["log_score"][0] == 1.2
    w = np.exp(score[0])
    assert np.allclose(r["marginal"][0], w / w.sum(), rtol=0, atol=1e-16) and abs(r["log_partition"][0] - np.log(w.sum())) < 1e-15
    r = hz.track_reference([0, 1], score, [2.0], [1.0], [0.0], 0.5, 1.0)
    assert r["cell"][0] == 3 and r["marginal"].shape == (1, 4)


def test_evidence_scores_and_empty_soundings():
    e = np.array([[1.0, 3.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    s, a = hz.evidence_scores(e)
    assert a is None and np.array_equal(s[1], np.zeros(3))                          # Z == 0: says nothing
    assert np.array_equal(s[0], np.log(np.maximum(e[0] / 4.0, 1e-6))) and s[0, 2] == np.log(1e-6) and s[2, 0] == 0.0
    s, a = hz.evidence_scores(e, absent=[4.0, 0.0, 0.0], floor=1e-3)
    assert np.array_equal(s[0], np.log(np.maximum(e[0] / 8.0, 1e-3))) and a[0] == np.log(0.5) and a[1] == 0.0 and a[2] == np.log(1e-3)
    st, at = hz.evidence_scores(torch.as_tensor(e), absent=torch.tensor([4.0, 0.0, 0.0]), floor=1e-3)
    assert isinstance(st, torch.Tensor) and np.array_equal(st.numpy(), s) and np.array_equal(at.numpy(), a)
    # an empty sounding in the middle of a line: the path passes through on the prior alone
    ev = np.zeros((3, 9))
    ev[0, 2] = ev[2, 4] = 1.0
    s, _ = hz.evidence_scores(ev)
    g, d = hz.steps([0.0, 10.0, 20.0], [0.0] * 3, [0.0] * 3, slope=0.05)
    r = hz.track_reference([0, 3], s, None, g, d, 0.5, 4.6)
    assert r["cell"][0] == 2 and r["cell"][2] == 4 and r["cell"][1] in (2, 3, 4)
    for bad in (-e, np.where(e == 3.0, np.nan, e), e[0]):
        with pytest.raises(ValueError):
            hz.evidence_scores(bad)
    with pytest.raises(ValueError):
        hz.evidence_scores(e, absent=[1.0])
    with pytest.raises(ValueError):
        hz.evidence_scores(e, floor=0.0)


def test_a_window_is_a_slice_of_the_state_axis():
    """Tracking the slice lo .. hi - 1 equals tracking the full axis where the other cells can never be entered."""
    rng = np.random.default_rng(5)
    N, S, lo, hi = 12, 10, 3, 8
    score, ab, g, d = _problem(rng, N, S, True)
    sl = hz.track_reference([0, N], score[:, lo:hi], ab, g, d, 0.5, 2.0)
    shut = np.full_like(score, -1.0e6)
    shut[:, lo:hi] = score[:, lo:hi]
    fu = hz.track_reference([0, N], shut, ab, g, d, 0.5, 2.0)
    cells = np.where(sl["cell"] == hi - lo, S, sl["cell"] + lo)
    assert np.array_equal(fu["cell"], cells) and fu["log_score"][0] == sl["log_score"][0]
    assert np.allclose(fu["marginal"][:, lo:hi], sl["marginal"][:, :-1], rtol=0, atol=1e-14)
    assert np.allclose(fu["marginal"][:, S], sl["marginal"][:, -1], rtol=0, atol=1e-14)
    assert fu["marginal"][:, :lo].max() == 0.0 and fu["marginal"][:, hi:S].max() == 0.0
    assert hz.window(np.arange(11) * 0.5, (1.5, 4.0)) == (3, 8) and hz.window(np.arange(11) * 0.5) == (0, 10)
    with pytest.raises(ValueError, match="no depth cell"):
        hz.window(np.arange(11) * 0.5, (1.3, 1.4))
    with pytest.raises(ValueError, match="d0 < d1"):
        hz.window(np.arange(11) * 0.5, (2.0, 1.0))


def test_steps_clamp_a_zero_distance():
    g, d = hz.steps([0.0, 0.0, 30.0, 30.0], [0.0, 0.0, 40.0, 40.5], [1.0, 3.0, 2.5, 2.5], slope=0.1, min_distance=2.0)
    assert np.array_equal(g, [1.0 / (0.1 * 2.0), 1.0 / (0.1 * 50.0), 1.0 / (0.1 * 2.0), 1.0 / (0.1 * 2.0)])
    assert np.array_equal(d, [2.0, -0.5, 0.0, 0.0])
    g, d = hz.steps([0.0, 10.0, 20.0, 50.0], [0.0] * 4, [0.0, 1.0, 5.0, 7.0], ptr=[0, 2, 4])          # no step across two sequences
    assert np.array_equal(d, [1.0, 0.0, 2.0, 0.0]) and g[1] == 1.0 / 0.05 and g[2] == 1.0 / (0.05 * 30.0)
    assert hz.steps([3.0], [4.0], [5.0])[0].shape == (1,)
    for kw in (dict(slope=0.0), dict(slope=-1.0), dict(min_distance=0.0), dict(slope=np.nan)):
        with pytest.raises(ValueError):
            hz.steps([0.0, 1.0], [0.0, 0.0], [0.0, 0.0], **kw)
    with pytest.raises(ValueError):
        hz.steps([0.0, 1.0], [0.0], [0.0, 0.0])
    with pytest.raises(ValueError):
        hz.steps([0.0, np.inf], [0.0, 0.0], [0.0, 0.0])
    with pytest.raises(ValueError):
        hz.steps([0.0, 1.0], [0.0, 0.0], [0.0, 0.0], ptr=[0, 1, 1, 2])


def test_as_intervals_and_files(tmp_path):
    top = dict(depth=torch.tensor([1.0, float("nan"), 3.0], dtype=torch.float64))
    iv = hz.as_intervals(top, np.array([4.0, 5.0, np.nan]))
    assert iv["kind"] == "horizons" and np.array_equal(iv["top"], [1.0, np.nan, 3.0], equal_nan=True)
    assert np.array_equal(iv["bottom"], [4.0, 5.0, np.nan], equal_nan=True)
    from geobipy_amd import intervals
    spec = intervals.check_spec(iv)
    rng = intervals.ranges(spec, np.arange(0.0, 10.5, 0.5), 3)
    assert list(rng.n_cells.reshape(-1)) == [6, 0, 0]                                 # a NaN pick gives that sounding no unit
    with pytest.raises(ValueError):
        hz.as_intervals(np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError):
        hz.as_intervals(np.zeros((3, 2)), np.zeros((3, 2)))
    res = dict(cell=torch.tensor([[1, -1]], dtype=torch.int32), depth=np.array([[0.75, np.nan]]), between=np.array([[0.0, 5.0]]))
    path = hz.save(res, str(tmp_path / "L.horizons.npz"))
    back = hz.load(path)
    assert set(back) == set(res) and np.array_equal(back["cell"], [[1, -1]]) and np.array_equal(back["depth"], res["depth"], equal_nan=True)
    assert hz.output_path("/a/b/100.0.h5") == "/a/b/100.0.horizons.npz" and hz.output_path("x.results.npz") == "x.horizons.npz"


def test_argument_checks():
    ev = torch.ones((4, 6), dtype=torch.float64)
    x, y, s, edges = np.arange(4.0), np.zeros(4), np.zeros(4), np.arange(7) * 0.5
    from geobipy_amd import _lib
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):        # a host tensor: there is no host path
        hz.track(ev, x, y, s, edges)
    with pytest.raises(ValueError, match="non-uniform"):
        hz.track(ev, x, y, s, np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.5]))
    with pytest.raises(ValueError, match="ascending"):
        hz.track(ev, x, y, s, edges[::-1])
    with pytest.raises(ValueError, match="depth cells"):
        hz.track(ev, x, y, s, np.arange(8) * 0.5)
    with pytest.raises(ValueError, match="one entry per sounding"):
        hz.track(ev, x[:3], y[:3], s[:3], edges)
    with pytest.raises(ValueError, match="switch"):
        hz.track(ev, x, y, s, edges, switch=-1.0)
    with pytest.raises(ValueError, match="slope"):
        hz.track(ev, x, y, s, edges, slope=0.0)
    with pytest.raises(ValueError, match="floor"):
        hz.track(ev, x, y, s, edges, floor=1.0)
    with pytest.raises(ValueError, match="absent"):
        hz.track(ev, x, y, s, edges, absent=torch.ones(3))
    with pytest.raises(ValueError, match="ptr"):
        hz.track(ev, x, y, s, edges, ptr=[0, 2, 2, 4])
    with pytest.raises(ValueError, match="ptr"):
        hz.track(ev, x, y, s, edges, ptr=[0, 3])
    with pytest.raises(ValueError, match="percentiles"):
        hz.track(ev, x, y, s, edges, percentiles=(0, 50))
    with pytest.raises(ValueError, match="torch tensor"):
        hz.track(np.ones((4, 6)), x, y, s, edges)
    with pytest.raises(ValueError, match="at most 2048"):
        hz.track(torch.ones((2, 2049), dtype=torch.float64), x[:2], y[:2], s[:2], np.arange(2050) * 0.5)
    with pytest.raises(ValueError, match="finite"):
        hz.track_reference([0, 2], [[0.0, np.inf], [0.0, 0.0]], None, [1.0, 1.0], [0.0, 0.0], 0.5, 1.0)
    with pytest.raises(ValueError, match="switch"):
        hz.track_reference([0, 2], np.zeros((2, 2)), None, [1.0, 1.0], [0.0, 0.0], 0.5, -1.0)
    with pytest.raises(ValueError, match="dz"):
        hz.track_reference([0, 2], np.zeros((2, 2)), None, [1.0, 1.0], [0.0, 0.0], 0.0, 1.0)
    with pytest.raises(ValueError, match="x, y and surface"):
        hz.from_products(dict(interface_probability=np.ones((4, 6)), interface_depth_edges=edges), [(0.0, 2.0)])
    with pytest.raises(ValueError, match="interface_probability"):
        hz.from_products(dict(mean=np.ones((4, 6))), [(0.0, 2.0)], x=x, y=y, surface=s)
    with pytest.raises(ValueError, match="first_hist"):
        hz.from_chains(dict(hitmap=None), x, y, s)


def test_command_line_parser():
    a = hz.parse_args(["out", "more/100.0.h5", "--between", "5", "40", "--between", "60", "120.5", "--slope", "0.02", "--no-marginals"])
    assert a.paths == ["out", "more/100.0.h5"] and a.between == [[5.0, 40.0], [60.0, 120.5]] and a.slope == 0.02 and a.switch == 4.6
    assert a.no_marginals and not a.absent and a.device is None
    a = hz.parse_args(["out", "--between", "0", "10", "--switch", "2.5", "--absent"])
    assert a.switch == 2.5 and a.absent and not a.no_marginals and a.slope == 0.05
    for bad in (["out"], ["out", "--between", "5"], ["out", "--between", "9", "3"], ["out", "--between", "1", "2", "--slope", "0"],
                ["out", "--between", "1", "2", "--switch", "-1"], ["--between", "1", "2"]):
        with pytest.raises(SystemExit):
            hz.parse_args(bad)


def _lib_or_skip():
    from geobipy_amd import _lib
    try:
        return _lib, _lib.load()
    except (_lib.NativeLibraryError, OSError) as e:
        pytest.skip("native library not loadable here: %s" % e)


def test_c_abi_refuses_bad_arguments():
    _lib, lib = _lib_or_skip()
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(L=2, ptr=p, total=5, max_n=3, S=4, dz=0.5, score=p, absent=None, g=p, d=p, switch=1.0, back=p, cell=p, log_score=p, marginal=None,
             log_partition=None, scale=None):
        return lib.gbp_horizon_track(L, ptr, total, max_n, S, dz, score, absent, g, d, switch, back, cell, log_score, marginal, log_partition,
                                     scale, None)

    err = lib.gbp_last_error
    # every one of these is refused before anything touches a device
    assert call(L=-1) == INVALID and b"gbp_horizon_track" in err() and b"L must" in err()
    assert call(S=0) == INVALID and call(S=2049) == INVALID and b"gbp_horizon_track" in err() and b"S must" in err()
    assert call(dz=0.0) == INVALID and call(dz=float("nan")) == INVALID and b"dz" in err()
    assert call(switch=-0.5) == INVALID and call(switch=float("nan")) == INVALID and b"switch" in err()
    for name in ("ptr", "score", "g", "d", "back", "cell", "log_score"):
        assert call(**{name: None}) == INVALID, name
        assert b"gbp_horizon_track" in err() and (b"NULL" in err()), name
    assert call(ptr=None) == INVALID and b"ptr" in err()
    assert call(back=None) == INVALID and b"back" in err()
    assert call(total=1) == INVALID and call(max_n=0) == INVALID and call(max_n=6) == INVALID and call(total=7) == INVALID
    assert b"total_n" in err()
    assert call(marginal=p) == INVALID and call(marginal=p, log_partition=p) == INVALID and call(scale=p) == INVALID and b"marginal" in err()
    # no sequences: no launch, whatever the pointers -- but the sizes are still checked
    assert call(L=0, ptr=None, total=0, max_n=0, score=None, g=None, d=None, back=None, cell=None, log_score=None) == 0
    assert call(L=0, S=0) == INVALID and call(L=0, switch=-1.0) == INVALID


def _planted(seed=0):
    rng = np.random.default_rng(seed)
    N, S, dz = 400, 120, 0.5
    x = 25.0 * np.arange(N)
    surface = 10.0 * np.sin(x / 1500.0) + rng.normal(0.0, 0.3, N)
    depth = surface - (-20.0 + 6.0 * np.sin(x / 2000.0))
    true = np.floor(depth / dz).astype(np.int64)
    assert true.min() >= 0 and true.max() < S
    at = np.where(rng.uniform(size=N) < 0.3, rng.integers(0, S, N), true)
    evidence = 0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2)
    return x, surface, true, evidence, dz


def test_a_planted_horizon_under_terrain():
    x, surface, true, evidence, dz = _planted()
    N, S = evidence.shape
    score, _ = hz.evidence_scores(evidence)
    g, d = hz.steps(x, np.zeros(N), surface, slope=0.05)
    r = hz.track_reference([0, N], score, None, g, d, dz, 4.6)
    err = np.abs(r["cell"] - true)
    naive = np.abs(np.argmax(evidence, axis=1) - true)
    lo, hi = (hz.percentile_cells(r["marginal"], p).numpy() for p in (5, 95))
    cover = np.mean((lo - 1 <= true) & (true <= hi + 1))
    print("tracked: max error %d cells, mean %.3f; argmax: max %d, %.1f %% off by more than 2; band covers %.1f %%, median width %g cells"
          % (err.max(), err.mean(), naive.max(), 100.0 * np.mean(naive > 2), 100.0 * cover, np.median(hi - lo + 1)))
    assert err.max() <= 4                                  # twice the width of the evidence's bump
    assert np.mean(naive > 2) >= 0.20                      # the evidence alone cannot pass
    assert cover >= 0.95
