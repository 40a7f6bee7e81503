"""The rule of the horizon pairs, horizons.unit_reference, on the host: against the enumeration of every path of a
tiny chain, against ``track_reference`` where the base is pinned, on a planted line where two tracks alone cross, and its refusals."""
import itertools

import numpy as np
import pytest

from geobipy_amd import horizons as hz

DZ, SWITCH = 0.5, 1.7


def _tiny(absent, thick, seed, S=4, N=4):
    rng = np.random.default_rng(seed)
    st, sb = rng.normal(0.0, 1.5, (N, S)), rng.normal(0.0, 1.5, (N, S))
    ab = rng.normal(0.0, 1.5, N) if absent else None
    ts = rng.normal(0.0, 1.0, S) if thick else None
    x = np.cumsum(rng.uniform(5.0, 30.0, N))
    surface = np.cumsum(rng.normal(0.0, 0.7, N))                             # steps that are no multiples of dz
    g, d = hz.steps(x, np.zeros(N), surface, slope=0.05)
    assert np.all(np.abs(d[:-1] / DZ - np.round(d[:-1] / DZ)) > 1e-3)
    return st, sb, ab, ts, g, d


def _enumerate(st, sb, ab, ts, g, d, mc):
    """Every path of the chain: its score, summed in the rule's order, and its states.  The absent state is (S, S)."""
    N, S = st.shape
    states = [(a, b) for a in range(S) for b in range(S) if b - a >= mc] + ([(S, S)] if ab is not None else [])
    T = lambda n, k: g[n] * np.abs(d[n] - np.float64(k) * DZ)               # noqa: E731

    def node(n, s):
        if s[0] == S:
            return ab[n]
        v = st[n, s[0]] + sb[n, s[1]]
        return v if ts is None else v + ts[s[1] - s[0]]

    paths, scores = [], []
    for p in itertools.product(states, repeat=N):
        v = node(0, p[0])
        for n in range(N - 1):
            (a, b), (a2, b2) = p[n], p[n + 1]
            if a < S and a2 < S:
                m = (v - T(n, a2 - a)) - T(n, b2 - b)
            elif a == S and a2 == S:
                m = v
            else:
                m = v - SWITCH
            v = node(n + 1, p[n + 1]) + m
        paths.append(p)
        scores.append(v)
    return paths, np.array(scores)


@pytest.mark.parametrize("mc", [0, 1, 2])
@pytest.mark.parametrize("absent", [False, True])
def test_the_rule_against_the_enumeration(absent, mc):
    S = N = 4
    st, sb, ab, ts, g, d = _tiny(absent, mc == 1, 10 + mc + 3 * absent)
    r = hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, min_cells=mc, thickness_score=ts, absent_score=ab)
    paths, scores = _enumerate(st, sb, ab, ts, g, d, mc)
    assert r["log_score"][0] == scores.max()                                 # the same operations in the same order: ==
    best = paths[int(np.argmax(scores))]
    if np.sum(scores == scores.max()) == 1:
        assert [tuple(v) for v in zip(r["cell_top"], r["cell_base"])] == list(best)
    assert r["cell_top"].dtype == np.int32 and r["cell_base"].dtype == np.int32
    w = np.exp(scores)
    Z = w.sum()
    top, base, thick, gone = np.zeros((N, S)), np.zeros((N, S)), np.zeros((N, S)), np.zeros(N)
    for p, wp in zip(paths, w):
        for n, (a, b) in enumerate(p):
            if a == S:
                gone[n] += wp
            else:
                top[n, a] += wp
                base[n, b] += wp
                thick[n, b - a] += wp
    for k, want in (("marginal_top", top), ("marginal_base", base), ("marginal_thickness", thick), ("marginal_absent", gone)):
        assert np.abs(r[k] - want / Z).max() <= 1e-12, k
    assert abs(r["log_partition"][0] - np.log(Z)) <= 1e-12
    assert np.abs(np.cumsum(np.log(r["scale"]))[-1] - r["log_partition"][0]) <= 1e-12
    assert np.all(r["marginal_thickness"][:, :mc] == 0.0)
    quick = hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, min_cells=mc, thickness_score=ts, absent_score=ab, marginals=False)
    assert set(quick) == {"cell_top", "cell_base", "log_score"} and np.array_equal(quick["cell_top"], r["cell_top"])


@pytest.mark.parametrize("terrain", [False, True])
def test_a_pinned_base_reduces_to_track(terrain):
    rng = np.random.default_rng(5)
    ptr, S = np.array([0, 1, 3, 14]), 9
    total = int(ptr[-1])
    st = rng.normal(0.0, 2.0, (total, S))
    sb = np.full((total, S), -1e6)
    sb[:, S - 1] = 0.0
    x = np.cumsum(rng.uniform(5.0, 30.0, total))
    surface = np.cumsum(rng.normal(0.0, 0.7, total)) if terrain else np.zeros(total)
    g, d = hz.steps(x, np.zeros(total), surface, slope=0.05, ptr=ptr)
    r = hz.unit_reference(ptr, st, sb, g, d, DZ, SWITCH, min_cells=0, marginals=False)
    one = hz.track_reference(ptr, st, None, g, d, DZ, SWITCH, marginals=False)
    assert np.array_equal(r["cell_top"], one["cell"]) and np.all(r["cell_base"] == S - 1)
    if not terrain:                                                          # the base's step costs exactly 0: the same sums
        assert np.array_equal(r["log_score"], one["log_score"])


def _planted():
    """A line of 16 soundings on flat ground, one cell of jump costs one nat: the top at cell 5 throughout; the base at cell 8, but on
    the stretch 5 .. 10 its evidence there is weak and a decoy at cell 2, above the top, is strong."""
    N, S, stretch = 16, 12, slice(5, 11)
    st, sb = np.full((N, S), -6.0), np.full((N, S), -6.0)
    st[:, 5] = 0.0
    sb[:, 8] = 0.0
    sb[stretch, 8] = -5.5
    sb[stretch, 2] = 0.0
    g, d = hz.steps(20.0 * np.arange(N), np.zeros(N), np.zeros(N), slope=0.05)
    return N, S, stretch, st, sb, g, d


@pytest.mark.parametrize("mc", [1, 2])
def test_the_planted_line_stays_ordered(mc):
    N, S, stretch, st, sb, g, d = _planted()
    top = hz.track_reference([0, N], st, None, g, d, 1.0, SWITCH, marginals=False)["cell"]
    base = hz.track_reference([0, N], sb, None, g, d, 1.0, SWITCH, marginals=False)["cell"]
    assert np.any(base[stretch] < top[stretch])                              # the precondition: tracked alone, the picks cross
    r = hz.unit_reference([0, N], st, sb, g, d, 1.0, SWITCH, min_cells=mc)
    assert np.all(r["cell_base"] - r["cell_top"] >= mc)
    assert np.all(r["cell_top"] == 5) and np.all(r["cell_base"] == 8)
    assert np.all(r["marginal_thickness"][:, :mc] == 0.0)
    mass = r["marginal_top"].sum(axis=1)
    assert np.abs(mass - 1.0).max() <= 1e-12 and np.abs(r["marginal_thickness"].sum(axis=1) - 1.0).max() <= 1e-12
    both = hz.unit_reference([0, N], st, sb, g, d, 1.0, SWITCH, min_cells=mc, absent_score=np.full(N, -3.0))
    here = both["cell_top"] < S
    assert np.array_equal(here, both["cell_base"] < S) and np.all((both["cell_base"] - both["cell_top"])[here] >= mc)
    assert np.abs(both["marginal_top"].sum(axis=1) + both["marginal_absent"] - 1.0).max() <= 1e-12


def test_refusals():
    N, S = 3, 4
    st, sb = np.zeros((N, S)), np.zeros((N, S))
    g, d = hz.steps(20.0 * np.arange(N), np.zeros(N), np.zeros(N))
    with pytest.raises(ValueError, match="min_cells"):
        hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, min_cells=S)
    with pytest.raises(ValueError, match="min_cells"):
        hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, min_cells=-1)
    bad = st.copy()
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        hz.unit_reference([0, N], bad, sb, g, d, DZ, SWITCH)
    with pytest.raises(ValueError, match="finite"):
        hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, absent_score=np.array([0.0, np.nan, 0.0]))
    with pytest.raises(ValueError, match="thickness_score"):
        hz.unit_reference([0, N], st, sb, g, d, DZ, SWITCH, thickness_score=np.zeros(S + 1))
    with pytest.raises(ValueError, match="score_top and score_base"):
        hz.unit_reference([0, N], st, sb[:, :3], g, d, DZ, SWITCH)
    with pytest.raises(ValueError, match="switch"):
        hz.unit_reference([0, N], st, sb, g, d, DZ, -1.0)
    assert hz.unit_bytes(10, 4) == 10 * (2 * 16 + 4) + 10 * 17 * 8 and hz.unit_bytes(10, 4, False) == 10 * 36
    assert hz.MAX_UNIT_STATES >= 96
