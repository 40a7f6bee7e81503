"""The host side of the joint draws of sections (geobipy_amd/sections.py draw_reference, philox_uniform, exceedance_area_reference;
DESIGN.md 3.26), on the rule alone: the draws' frequencies against the exact probability of every path and against the smoothed
marginals, the filter against the formulas, what a draw depends on (seed, realisation, row key -- not R, not the grouping into calls),
the degenerate shapes, the random numbers against the sampler's emulation, the area product on a hand-made section, and every refusal.

The statistical bound.  A count of R draws with probability p has standard deviation sqrt(R p (1 - p)); the tests hold every compared
cell within 5 of them.  With a few hundred cells at 5.7e-7 each (the two-sided normal tail at 5 sigma) a correct rule fails with
probability < 1e-3 -- and the seeds are fixed, so a run repeats.  Every case prints its worst |z|."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rj_emul
from geobipy_amd import _lib, ensembles, sections

R_STAT = 4096


def ragged_chain(seed, n, N, ones=(3,)):
    """One sequence of N soundings with up to n models: ragged n_used (1 at the soundings ``ones``, n at the first), NaN outside the
    prefixes and in the last sounding's entry."""
    rng = np.random.default_rng(seed)
    n_used = rng.integers(2, n + 1, N).astype(np.int32)
    n_used[0] = n
    n_used[list(ones)] = 1
    score, g, d2 = rng.normal(0.0, 0.7, (N, n)), rng.uniform(0.5, 2.0, N), rng.uniform(0.0, 1.5, (N, n, n))
    for r in range(N):
        d2[r, n_used[r]:, :] = np.nan
        if r + 1 < N:
            d2[r, :, n_used[r + 1]:] = np.nan
    d2[N - 1] = np.nan
    return np.array([0, N]), score, g, d2, n_used


def worst_z(observed, p, R, least):
    """(the worst |observed - R p| / sqrt(R p (1 - p)) over the cells with R p >= 5, their number); asserts at least ``least`` cells.
    A cell of probability 1 has no spread: it must hold every draw, and is not counted."""
    p = np.asarray(p, dtype=np.float64)
    assert np.all(observed[p == 1.0] == R)
    cells = (R * p >= 5.0) & (p < 1.0)
    assert int(cells.sum()) >= least, int(cells.sum())
    z = np.abs(observed[cells] - R * p[cells]) / np.sqrt(R * p[cells] * (1.0 - p[cells]))
    return float(z.max()), int(cells.sum())


def check_marginal_frequencies(draw_state, marginal, n_used, R, what):
    """The per-sounding frequencies of ``draw_state`` [R, N] against ``marginal`` [N, n] within 5 sigma, on at least 30 cells."""
    N, n = marginal.shape
    counts = np.stack([np.bincount(draw_state[:, s], minlength=n) for s in range(N)])
    z, cells = worst_z(counts, marginal, R, 30)
    print("%s: worst |z| = %.2f over %d cells" % (what, z, cells))
    assert z <= 5.0
    for s in range(N):
        assert counts[s, n_used[s]:].sum() == 0


# ---- the joint law ------------------------------------------------------------------------------------------------------------------

def test_paths_are_drawn_with_their_exact_probabilities():
    rng = np.random.default_rng(5)
    n, n_used = 3, np.array([3, 1, 3, 3], dtype=np.int32)
    ptr, score, g = np.array([0, 4]), rng.normal(0.0, 0.5, (4, n)), rng.uniform(0.5, 1.5, 4)
    d2 = rng.uniform(0.0, 1.5, (4, n, n))
    d2[2, 0, 0] = 1.0e5                                                       # exp(-(g d2)) underflows to 0.0: three paths of probability 0
    d2[0, :, 1:] = d2[1, 1:, :] = d2[3] = np.nan
    paths = list(itertools.product(*[range(int(m)) for m in n_used]))
    lw = np.array([sum(np.longdouble(score[s, p[s]]) for s in range(4)) - sum(np.longdouble(g[s]) * np.longdouble(d2[s, p[s], p[s + 1]]) for s in range(3))
                   for p in paths])
    prob = np.exp(lw) / np.exp(lw).sum()
    assert (prob == 0).sum() == 3 and len(paths) == 27
    out = sections.draw_reference(ptr, score, g, d2, n_used, R_STAT, seed=11)
    ds = out["draw_state"]
    assert ds.dtype == np.int32 and ds.shape == (R_STAT, 4) and out["margin"].shape == (R_STAT, 4) and out["filtered"].shape == (4, n)
    index = {p: q for q, p in enumerate(paths)}
    counts = np.bincount([index[tuple(row)] for row in ds.tolist()], minlength=len(paths))
    z, cells = worst_z(counts, prob, R_STAT, 20)
    print("paths: worst |z| = %.2f over %d paths" % (z, cells))
    assert z <= 5.0
    assert counts[prob == 0].sum() == 0                                        # a path of probability 0 is never drawn
    assert np.all(out["margin"] >= 0) and np.all(out["margin"] <= 1)


def test_frequencies_match_the_smoothed_marginals():
    ptr, score, g, d2, n_used = ragged_chain(21, 6, 12)
    ld = sections.track_reference(ptr, score, g, d2, n_used, dtype=np.longdouble)
    out = sections.draw_reference(ptr, score, g, d2, n_used, R_STAT, seed=3)
    check_marginal_frequencies(out["draw_state"], ld["marginal"].astype(np.float64), n_used, R_STAT, "rule, n = 6, N = 12")


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_filtered_is_the_alpha_of_the_rule(dtype):
    ft = np.dtype(dtype).type
    ptr, score, g, d2, n_used = ragged_chain(8, 5, 7, ones=(2,))
    out = sections.draw_reference(ptr, score, g, d2, n_used, 3, dtype=dtype)
    N, n = score.shape
    alpha = np.zeros((N, n), dtype=ft)
    w = np.exp(score.astype(ft))
    alpha[0, :n_used[0]] = w[0, :n_used[0]] / w[0, :n_used[0]].sum()
    for s in range(N - 1):
        m, mn = int(n_used[s]), int(n_used[s + 1])
        u = np.zeros(mn, dtype=ft)
        for i in range(m):
            u = u + alpha[s, i] * np.exp(-(g[s].astype(ft) * d2[s, i, :mn].astype(ft)))
        u = w[s + 1, :mn] * u
        alpha[s + 1, :mn] = u / u.sum()
    assert out["filtered"].dtype == ft and np.array_equal(out["filtered"], alpha)
    both = sections.track_reference(ptr, score, g, d2, n_used, dtype=dtype)   # the scale of the existing rule: the same sums
    assert np.array_equal(both["scale"][0], w[0, :n_used[0]].sum())


# ---- what a draw depends on -----------------------------------------------------------------------------------------------------------

def test_the_first_draws_do_not_depend_on_how_many_are_drawn():
    ptr, score, g, d2, n_used = ragged_chain(2, 5, 9)
    few, many = (sections.draw_reference(ptr, score, g, d2, n_used, R, seed=2 ** 40 + 5) for R in (37, 100))
    assert np.array_equal(few["draw_state"], many["draw_state"][:37]) and np.array_equal(few["margin"], many["margin"][:37])
    other = sections.draw_reference(ptr, score, g, d2, n_used, 37, seed=2 ** 40 + 6)
    assert not np.array_equal(few["draw_state"], other["draw_state"])          # the seed is used, high word included
    assert not np.array_equal(few["draw_state"], sections.draw_reference(ptr, score, g, d2, n_used, 37, seed=5)["draw_state"])


def test_keys_decide_a_draw_not_positions():
    ptr, score, g, d2, n_used = ragged_chain(4, 4, 9, ones=(6,))
    key = np.array([90, 7, 2 ** 33 + 1, 5, 12, 2 ** 40, 3, 77, 8], dtype=np.int64)
    cut = sections.draw_reference([0, 4, 9], score, g, d2, n_used, 50, seed=9, row_key=key)
    alone = sections.draw_reference([0, 5], score[4:], g[4:], d2[4:], n_used[4:], 50, seed=9, row_key=key[4:])
    assert np.array_equal(cut["draw_state"][:, 4:], alone["draw_state"]) and np.array_equal(cut["filtered"][4:], alone["filtered"])
    by_position = sections.draw_reference([0, 5], score[4:], g[4:], d2[4:], n_used[4:], 50, seed=9)
    assert np.array_equal(by_position["draw_state"], sections.draw_reference([0, 5], score[4:], g[4:], d2[4:], n_used[4:], 50, seed=9, row_key=np.arange(5))["draw_state"])
    assert not np.array_equal(by_position["draw_state"], alone["draw_state"])


def test_one_sounding_and_one_model():
    rng = np.random.default_rng(1)
    score = rng.normal(0.0, 1.0, (3, 4))
    out = sections.draw_reference([0, 1, 1, 2, 3], score, np.ones(3), np.full((3, 4, 4), np.nan), [4, 2, 1], 2000, seed=1)      # N = 1 three times, one empty sequence
    w = np.exp(score[0])
    assert np.array_equal(out["filtered"][0], w / w.sum()) and np.all(out["draw_state"][:, 2] == 0) and np.all(out["draw_state"][:, 1] < 2)
    z, _ = worst_z(np.bincount(out["draw_state"][:, 0], minlength=4), w / w.sum(), 2000, 4)
    assert z <= 5.0
    one = sections.draw_reference([0, 5], None, np.ones(5), np.zeros((5, 1, 1)), np.ones(5, dtype=np.int32), 7)      # n = 1
    assert not one["draw_state"].any() and np.all(one["filtered"] == 1.0) and one["draw_state"].shape == (7, 5)
    none = sections.draw_reference([0], None, np.zeros(0), np.zeros((0, 2, 2)), np.zeros(0, dtype=np.int32), 3)
    assert none["draw_state"].shape == (3, 0) and none["filtered"].shape == (0, 2)


def test_philox_uniform_is_the_samplers_generator():
    for seed, draw, key in ((0, 0, 0), (1, 2, 3), (0xDEADBEEF12345678, 65535, 2 ** 32), (2 ** 63 + 17, 4095, 2 ** 40 + 123456789), (7, 1, 2 ** 62 + 5),
                            (2 ** 64 - 1, 9, 0xFFFFFFFF)):
        x = rj_emul.philox(seed, draw, key & 0xFFFFFFFF, key >> 32, 0)
        assert float(sections.philox_uniform(seed, draw, key)) == rj_emul.u53(x[0], x[1]), (seed, draw, key)
    draws, keys = np.arange(5)[:, None], np.array([0, 2 ** 32 + 1, 2 ** 45])[None, :]
    u = sections.philox_uniform(2 ** 35 + 1, draws, keys)
    assert u.shape == (5, 3) and u.dtype == np.float64 and np.all((u >= 0) & (u < 1))
    for a in range(5):
        for b in range(3):
            x = rj_emul.philox(2 ** 35 + 1, a, int(keys[0, b]) & 0xFFFFFFFF, int(keys[0, b]) >> 32, 0)
            assert u[a, b] == rj_emul.u53(x[0], x[1])
    for bad in (-1, 2 ** 64, 1.0, True):
        with pytest.raises(ValueError, match="seed"):
            sections.philox_uniform(bad, 0, 0)


# ---- the area product -----------------------------------------------------------------------------------------------------------------

def hand_made_section():
    """Two sequences (three soundings at x = 0, 10, 30; one at 100), two realisations; realisation 1 has no model under sounding 1.
    Widths 10, 15, 20 and 0; window 5 .. 25 m, threshold 0.1 S/m: sounding 0 has a layer 4 .. 30 m straddling both ends of the window."""
    inf, nan = np.inf, np.nan
    k = np.array([[3, 1, 2, 2], [3, 0, 2, 2]], dtype=np.int32)
    edges = np.array([[[4.0, 30.0, inf], [inf, inf, inf], [10.0, inf, inf], [8.0, inf, inf]]] * 2)
    sigma = np.array([[[1.0, 0.5, 0.01], [0.2, nan, nan], [0.05, 0.3, nan], [1.0, 1.0, nan]]] * 2)
    edges[1, 1], sigma[1, 1] = nan, nan
    return k, edges, sigma, np.array([0.0, 10.0, 30.0, 100.0]), np.zeros(4), np.array([0, 3, 4])


def test_exceedance_area_on_a_hand_made_section():
    k, edges, sigma, x, y, ptr = hand_made_section()
    assert sections.section_widths(x, y, ptr).tolist() == [10.0, 15.0, 20.0, 0.0]
    assert sections.section_widths(x, y).tolist() == [10.0, 15.0, 45.0, 70.0] and sections.section_widths([], []).size == 0
    above = sections.exceedance_area_reference(k, edges, sigma, x, y, ptr, 0.1, 5.0, 25.0)
    assert above.tolist() == [[800.0, 0.0], [500.0, 0.0]]                      # 10 * 20 + 15 * 20 + 20 * 15; the sequence of one sounding has no width
    below = sections.exceedance_area_reference(k, edges, sigma, x, y, ptr, 0.1, 5.0, 25.0, above=False)
    assert below.tolist() == [[100.0, 0.0], [100.0, 0.0]]                      # 20 * (10 - 5): with the above, the window's 45 * 20 where there are models
    for ab, want in ((True, above), (False, below)):                           # plain torch: the same numbers on any device
        got = sections.exceedance_area(torch.as_tensor(k), torch.as_tensor(edges), torch.as_tensor(sigma), x, y, ptr, 0.1, 5.0, 25.0, above=ab)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    one = sections.exceedance_area_reference(k, edges, sigma, x, y, None, 0.1, 5.0, 25.0)
    assert one.tolist() == [[10 * 20 + 15 * 20 + 45 * 15 + 70 * 20.0], [10 * 20 + 45 * 15 + 70 * 20.0]]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_by_message(capsys):
    d2, g, ptr, n_used = torch.zeros((3, 4, 4), dtype=torch.float64), np.ones(3), [0, 3], np.array([4, 1, 2])
    ref = lambda d2_, g_, p_, nu_, R, **kw: sections.draw_reference(p_, kw.pop("score", None), g_, d2_, nu_, R, **kw)      # noqa: E731
    for draw in (sections.draw, ref):
        for bad, match in (((d2[0], g, ptr, n_used, 2), "d2"), ((d2[:, :3], g, ptr, n_used, 2), "d2"), ((d2, g[:2], ptr, n_used, 2), "g must"),
                           ((d2, g, [0, 2], n_used, 2), "ptr"), ((d2, g, [0, 2, 1, 3], n_used, 2), "not decrease"), ((d2, g, ptr, n_used[:2], 2), "n_used"),
                           ((d2, g, ptr, np.array([4, 0, 2]), 2), "1 .. n"), ((d2, g, ptr, np.array([4, 5, 2]), 2), "1 .. n"),
                           ((d2, g, ptr, n_used, 0), "n_draws"), ((d2, g, ptr, n_used, 65537), "n_draws"), ((d2, g, ptr, n_used, 2.0), "n_draws")):
            with pytest.raises(ValueError, match=match):
                draw(*bad)
        for kw, match in ((dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=0.5), "seed"), (dict(row_key=np.arange(2)), "row_key"),
                          (dict(row_key=np.zeros(3)), "row_key"), (dict(score=torch.zeros((3, 3), dtype=torch.float64)), "score")):
            with pytest.raises(ValueError, match=match):
                draw(d2, g, ptr, n_used, 2, **kw)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.draw(d2.numpy(), g, ptr, n_used, 2)
    with pytest.raises(TypeError):
        sections.draw(d2.float(), g, ptr, n_used, 2)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_draw"):     # host tensors: refused after the shape, dtype and value checks
        sections.draw(d2, g, ptr, n_used, 2, row_key=np.arange(3))

    k = torch.ones((2, 8), dtype=torch.int32)
    ens = ensembles.Ensemble(k, torch.full((2, 8, 4), float("inf"), dtype=torch.float64), torch.ones((2, 8, 4), dtype=torch.float64),
                             torch.zeros((2, 8), dtype=torch.float64), (k > 0).sum(dim=1), 1, torch.zeros(2, dtype=torch.float64))
    x = y = np.zeros(2)
    for kw, match in ((dict(draws=-1), "draws"), (dict(draws=65537), "draws"), (dict(draws=1.5), "draws"), (dict(draws=2, seed=-3), "seed")):
        with pytest.raises(ValueError, match=match):
            sections.sections(ens, x, y, 10.0, **kw)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.sections(ens, x, y, 10.0, draws=2)
    slot = torch.zeros((3, 2), dtype=torch.int32)
    for bad in (slot[0], slot[:, :1], slot[:0], slot.long()):
        with pytest.raises(ValueError, match="draw_slot"):
            sections.draw_models(ens, bad)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.draw_models(ens, slot.numpy())
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.draw_models(ens, slot)

    kk, edges, sigma, xs, ys, p = hand_made_section()
    t = lambda a: torch.as_tensor(a)                                           # noqa: E731
    for args, match in (((kk, t(edges), t(sigma), xs, ys, p, 0.1, 5.0, 25.0), "torch tensors"), ((t(kk), t(edges)[:, :3], t(sigma), xs, ys, p, 0.1, 5.0, 25.0), "R, S, K"),
                        ((t(kk), t(edges), t(sigma), xs, ys, p, float("nan"), 5.0, 25.0), "threshold"), ((t(kk), t(edges), t(sigma), xs, ys, p, 0.1, 25.0, 5.0), "z0 < z1"),
                        ((t(kk), t(edges), t(sigma), xs, ys, p, 0.1, -1.0, 5.0), "z0 < z1"), ((t(kk), t(edges), t(sigma), xs, ys, [0, 5], 0.1, 5.0, 25.0), "ptr"),
                        ((t(kk), t(edges), t(sigma), xs[:3], ys[:3], p, 0.1, 5.0, 25.0), "one entry per sounding")):
        with pytest.raises(ValueError, match=match):
            sections.exceedance_area(*args)

    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--draws", "4", "--seed", "3"])
    assert kw["draws"] == 4 and kw["seed"] == 3
    assert "draws" not in sections.parse_args(["run.npz", "--depth", "150"])[1]
    for argv in (["run.npz", "--depth", "10", "--draws", "-1"], ["run.npz", "--depth", "10", "--draws", "70000"], ["run.npz", "--depth", "10", "--draws", "2", "--seed", "-1"]):
        with pytest.raises(SystemExit):
            sections.parse_args(argv)
    capsys.readouterr()
    assert len(_lib.SIGNATURES["gbp_section_draw"][1]) == 15
