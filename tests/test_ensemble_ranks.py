"""The rule of the ranks (geobipy_amd.ensembles.rank_counts_reference: less / leq counts with ties, order statistics, folding;
DESIGN.md 3.24) and of the rank diagnostics built on it (rank_diagnostics_reference) on the host: against scipy's midranks and
numpy's quantiles on continuous, tied and extreme columns, the empty and non-finite cases, invariance under monotone maps, what
bulk / folded / tail statistics say about series whose answer is known, Spearman's correlation, and the refusals every entry makes
before the library loads."""
import numpy as np
import pytest

from geobipy_amd import ensembles
from geobipy_amd.ensembles import rank_counts_reference as rule

U = 2.0 ** -52
PROBS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0)


def columns(rng, n):
    """The columns every rank test uses, [n, 8]: continuous, runs of 8 equal values, three distinct values, 97 % tied, all equal, +-0.0
    mixed, denormals, +-1.7e308 (folded to +inf)."""
    c = np.empty((n, 8))
    c[:, 0] = rng.standard_normal(n)
    c[:, 1] = np.repeat(rng.standard_normal((n + 7) // 8), 8)[:n]
    c[:, 2] = rng.choice([-1.5, 0.25, 7.0], size=n)
    c[:, 3] = np.where(rng.random(n) < 0.97, 0.5, rng.standard_normal(n))
    c[:, 4] = 3.25
    c[:, 5] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    c[:, 6] = rng.integers(-3, 4, size=n) * (1024 * 4.9e-324)            # (1 024 apart: an interpolated quantile does not round onto s[lo + 1])
    c[:, 7] = np.where(rng.random(n) < 0.5, 1.7e308, -1.7e308)
    return c


def used_rows(starts, n):
    return np.concatenate([np.arange(q, q + n) for q in starts])


@pytest.mark.parametrize("starts, n", [((0,), 64), ((3, 40), 33), ((0, 7), 7), ((2, 50, 100, 150), 43), ((0, 4), 4)])
def test_counts_are_scipys_midranks_and_numpys_quantiles(starts, n):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    x = columns(rng, max(starts) + n + 5)
    rows, nu = used_rows(starts, n), len(starts) * n
    got = rule(x, starts, n, probabilities=PROBS)
    less, leq, order = got["less"], got["leq"], got["order"]
    unused = np.setdiff1d(np.arange(x.shape[0]), rows)
    assert less.dtype == np.int32 and leq.dtype == np.int32 and order.shape == (len(PROBS), 2, 8)
    assert np.all(less[unused] == -1) and np.all(leq[unused] == -1)
    assert np.all(less[rows] >= 0) and np.all(less[rows] < leq[rows]) and np.all(leq[rows] <= nu)
    for v in range(8):
        c = x[rows, v]
        assert np.array_equal((less[rows, v] + leq[rows, v] + 1) / 2, stats.rankdata(c, method="average"))
        assert np.array_equal(less[rows, v], (c[None, :] < c[:, None]).sum(axis=1)) and np.array_equal(leq[rows, v], (c[None, :] <= c[:, None]).sum(axis=1))
        for i, p in enumerate(PROBS):
            lo = np.floor((nu - 1) * p)
            g = (nu - 1) * p - lo
            with np.errstate(over="ignore", invalid="ignore"):
                q = order[i, 0, v] + g * (order[i, 1, v] - order[i, 0, v])
                want = np.quantile(c, p)
            if v == 7:                                                   # (+1.7e308) - (-1.7e308) overflows in both formulas
                with np.errstate(over="ignore"):
                    crossing = not np.isfinite(order[i, 1, v] - order[i, 0, v])
                assert q == want or crossing
                assert crossing or np.array_equal(less[rows, v] <= lo, c <= want)
            else:
                assert abs(q - want) <= 2 * U * abs(want) + (2 * 4.9e-324 if v == 6 else 0.0)
                assert np.array_equal(less[rows, v] <= lo, c <= want)    # I_p is I(x <= Q_p), ties included


def test_folding_and_both_parities_of_the_median():
    rng = np.random.default_rng(6)
    infinities = 0
    for starts, n in (((0, 20), 7), ((0, 20), 8), ((1,), 9)):
        x = columns(rng, 40)
        rows, nu = used_rows(starts, n), len(starts) * n
        got = rule(x, starts, n, fold=True, probabilities=(0.5,))
        plain = rule(x, starts, n, probabilities=(0.5,))
        assert np.array_equal(got["order"], plain["order"])             # taken before folding
        for v in range(8):
            c = x[rows, v]
            s = np.sort(c)
            with np.errstate(over="ignore"):
                med = 0.5 * (s[(nu - 1) // 2] + s[nu // 2])              # (1.7e308 + 1.7e308: the rule's median is +inf then)
                f = np.abs(c - med)
            assert med == np.median(c) or v == 7
            infinities += int(np.isinf(f).sum()) if v == 7 else 0
            assert np.array_equal(got["less"][rows, v], (f[None, :] < f[:, None]).sum(axis=1))
            assert np.array_equal(got["leq"][rows, v], (f[None, :] <= f[:, None]).sum(axis=1))
    assert infinities > 0                                                # folded values that are +inf were ranked, ties among them


def test_empty_and_non_finite_cases():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((30, 3))
    for starts, n in (((), 10), ((0, 10), 3)):                           # M == 0, N == 3
        got = rule(x, starts, n, probabilities=(0.5,))
        assert np.all(got["less"] == -1) and np.all(got["leq"] == -1) and np.isnan(got["order"]).all()
    starts, n = (2, 16), 10
    rows = used_rows(starts, n)
    clean = rule(x, starts, n, fold=True, probabilities=(0.1, 0.9))
    y = x.copy()
    y[0, 1] = np.nan                                                     # an unused row: nothing changes
    y[28, 2] = np.inf
    got = rule(y, starts, n, fold=True, probabilities=(0.1, 0.9))
    assert all(np.array_equal(got[k_], clean[k_]) for k_ in ("less", "leq", "order"))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17, 1] = bad                                                   # a used row
        got = rule(y, starts, n, probabilities=(0.1, 0.9))
        assert np.all(got["less"][:, 1] == -1) and np.all(got["leq"][:, 1] == -1) and np.isnan(got["order"][:, :, 1]).all()
        for v in (0, 2):
            assert np.array_equal(got["less"][:, v], rule(x, starts, n)["less"][:, v]) and np.isfinite(got["order"][:, :, v]).all()
        assert np.all(got["less"][rows, 0] >= 0)
    with pytest.raises(ValueError, match="overlap"):
        rule(x, (0, 5, 10, 15), 10)
    with pytest.raises(ValueError, match="leaves the rows"):
        rule(x, (25,), 10)
    for bad in ((-0.1,), (1.5,), (np.nan,), tuple([0.5] * 17), ((0.5,),)):
        with pytest.raises(ValueError):
            rule(x, starts, n, probabilities=bad)


def test_unfolded_products_are_invariant_under_monotone_maps():
    """exp and the cube are injective in fp64 on these values, so the counts -- and every product made of them -- are equal; the raw
    rhat and ess are not."""
    rng = np.random.default_rng(8)
    starts, n = (0, 64, 128, 192), 64
    x = np.round(np.cumsum(rng.standard_normal((256, 4)), axis=0) * 0.3, 3)
    x[rng.integers(0, 256, 40), 1] = x[0, 1]                             # some exact ties
    assert all(np.unique(f(x)).size == np.unique(x).size for f in (np.exp, lambda a: a ** 3))
    want = ensembles.rank_diagnostics_reference(x, starts, n, 63)
    raw = ensembles.diagnostics_reference(x, starts, n, 63)
    for f in (np.exp, lambda a: a ** 3):
        y = f(x)
        a, b = rule(x, starts, n, probabilities=(0.05, 0.5, 0.95)), rule(y, starts, n, probabilities=(0.05, 0.5, 0.95))
        assert np.array_equal(a["less"], b["less"]) and np.array_equal(a["leq"], b["leq"]) and np.array_equal(f(a["order"]), b["order"])
        got = ensembles.rank_diagnostics_reference(y, starts, n, 63)
        for name in ("rhat_bulk", "ess_bulk", "tau_bulk", "truncated_bulk", "ess_percentile_5", "ess_percentile_50", "ess_percentile_95", "ess_tail"):
            assert np.array_equal(got[name], want[name], equal_nan=True), name
        moved = ensembles.diagnostics_reference(y, starts, n, 63)
        assert not np.array_equal(moved["rhat"], raw["rhat"]) and not np.array_equal(moved["ess"], raw["ess"])


def test_what_the_rank_diagnostics_say_about_known_series():
    rng = np.random.default_rng(2021)
    starts, n, nu = (0, 64, 128, 192), 64, 256
    iid = rng.standard_normal((256, 1))
    ar = np.empty((256, 1))
    e = rng.standard_normal(256)
    for m in range(4):                                                   # four AR(1) chains, coefficient 0.9, started in equilibrium
        t0 = m * 64
        ar[t0, 0] = e[t0] / np.sqrt(1.0 - 0.81)
        for t in range(t0 + 1, t0 + 64):
            ar[t, 0] = 0.9 * ar[t - 1, 0] + e[t]
    spread = rng.standard_normal((256, 1))
    spread[128:] *= 3.0                                                  # equal medians, spreads 1 and 3
    d_iid, d_ar, d_sp = (ensembles.rank_diagnostics_reference(a, starts, n, 63) for a in (iid, ar, spread))
    print("ess_bulk iid", d_iid["ess_bulk"], "ar", d_ar["ess_bulk"], "rhat folded / bulk", d_sp["rhat_folded"], d_sp["rhat_bulk"])
    assert d_iid["ess_bulk"][0] >= nu / 2
    assert d_ar["ess_bulk"][0] <= nu / 4
    assert d_sp["rhat_folded"][0] > d_sp["rhat_bulk"][0]
    assert np.array_equal(d_sp["rhat_rank"], np.maximum(d_sp["rhat_bulk"], d_sp["rhat_folded"]))
    assert d_iid["ess_tail"][0] == min(d_iid["ess_percentile_5"][0], d_iid["ess_percentile_95"][0]) and np.isfinite(d_iid["ess_tail"][0])
    assert d_iid["quantile_50"][0] == np.quantile(iid[:, 0], 0.5)
    # a percentile on the sample's extreme: I_p is constant, its ESS NaN, and so is the tail's
    tied = np.where(np.arange(256) % 8 == 0, 1.0, 0.0)[:, None] + np.zeros((256, 1))      # 12.5 % of the values are the maximum
    d = ensembles.rank_diagnostics_reference(tied, starts, n, 63)
    assert np.isnan(d["ess_percentile_95"][0]) and np.isnan(d["ess_tail"][0]) and np.isfinite(d["ess_percentile_5"][0])
    # other percentiles give other names; the tail is made of the lowest and the highest
    d = ensembles.rank_diagnostics_reference(iid, starts, n, 63, percentiles=(2.5, 97.5))
    assert d["ess_tail"][0] == min(d["ess_percentile_2.5"][0], d["ess_percentile_97.5"][0]) and "quantile_2.5" in d


def test_spearman_through_the_correlation_rule():
    stats = pytest.importorskip("scipy.stats")
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    starts, n = (0, 40), 40
    x = np.cumsum(rng.standard_normal((80, 5)), axis=0)
    x[:, 3] = np.round(x[:, 3])                                          # ties
    r = rule(x, starts, n)
    mid = ensembles.midranks(torch.as_tensor(r["less"]), torch.as_tensor(r["leq"])).numpy()
    band = ensembles.correlation_reference(mid, starts, n, 4)["band"]
    want = stats.spearmanr(x).statistic
    for c in range(5):
        for j in range(5 - c):
            assert abs(band[c, j] - want[c, c + j]) <= 8 * U


def test_refusals_before_the_library_loads(monkeypatch):
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib, survey, survey_run
    from geobipy_amd.__main__ import parse

    def boom():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", boom)
    # the survey driver and its command line
    for kw in (dict(ensemble_rank_diagnostics=True), dict(ensemble_rank_diagnostics=dict(max_lag=7)), dict(ensemble_rank_diagnostics=True, ensemble=False)):
        with pytest.raises(ValueError, match="needs ensemble"):
            survey.infer("no such options file", **kw)
    for bad in (dict(max_lag=0), dict(max_lag=256), dict(lag=3), dict(percentiles=(50, 5)), dict(percentiles=(101,)), dict(percentiles=()),
                dict(percentiles=tuple(range(17))), 7, "yes"):
        with pytest.raises(ValueError):
            survey.infer("no such options file", ensemble=16, ensemble_rank_diagnostics=bad)
    arg = survey_run.ensemble_rank_diagnostics_argument
    assert arg(False, None) is None and arg(None, 16) is None
    assert arg(True, 16) == dict(max_lag=255, percentiles=(5.0, 50.0, 95.0))
    assert arg(dict(max_lag=31, percentiles=[10, 90]), dict(n_keep=8, thin=1)) == dict(max_lag=31, percentiles=(10.0, 90.0))
    with pytest.raises(SystemExit):
        parse(["options", "out", "--ensemble-rank-diagnostics"])
    with pytest.raises(SystemExit):
        parse(["options", "out", "--ensemble", "16", "--ensemble-rank-diagnostics", "256"])
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-rank-diagnostics"]).ensemble_rank_diagnostics == 255
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-rank-diagnostics", "31"]).ensemble_rank_diagnostics == 31
    assert parse(["options", "out", "--ensemble", "16"]).ensemble_rank_diagnostics is None
    # the command line of the module
    axis = ["run.npz", "--depth-axis", "40", "2.5"]
    assert ensembles.parse_rank(axis) == (None, False)
    assert ensembles.parse_rank(axis + ["--rank"]) == ((5.0, 50.0, 95.0), False)
    assert ensembles.parse_rank(axis + ["--rank", "--percentiles", "2.5", "97.5"]) == ((2.5, 97.5), False)
    assert ensembles.parse_rank(axis + ["--correlation", "--spearman"]) == (None, True)
    assert ensembles.rank_diagnostics_path("a/run.npz") == "a/run.rank_diagnostics.npz"
    for bad in (["--percentiles", "5"], ["--spearman"], ["--rank", "--spearman"], ["--rank", "--correlation"], ["--rank", "--percentiles", "95", "5"],
                ["--rank", "--percentiles", "120"]):
        with pytest.raises(SystemExit):
            ensembles.parse_rank(axis + bad)
    # the Python entries on an ensemble
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)      # noqa: E731
    B, ns, K = 2, 12, 5
    ens = dict(k=torch.ones((B, ns), dtype=torch.int32), edges=torch.full((B, ns, K), float("inf"), dtype=torch.float64), sigma=f64(B, ns, K) + 1.0,
               misfit=f64(B, ns) + 1.0, count=torch.full((B,), ns), thin=3, log_mean_prior=f64(B))
    edges = np.arange(11.0)
    E = lambda **kw: ensembles.Ensemble(**dict(ens, **kw))      # noqa: E731
    entries = (lambda e, **kw: ensembles.rank_diagnostics(e, edges, **kw), lambda e, **kw: ensembles.quantiles(e, edges, (5, 95), **kw),
               lambda e, **kw: ensembles.ensemble_ranks(e, edges, **kw), lambda e, **kw: ensembles.correlation(e, edges, rank=True, **kw))
    for entry in entries:
        with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
            entry(E())
        with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
            entry(E(k=ens["k"].numpy()))
        for kw in (dict(chains=5), dict(chains=0), dict(chains=9)):
            with pytest.raises(ValueError):
                entry(E(), **kw)
        for bad, error in ((dict(k=ens["k"].long()), TypeError), (dict(sigma=f64(B, ns, K + 1)), ValueError), (dict(edges=f64(B, ns, 65), sigma=f64(B, ns, 65)), ValueError)):
            with pytest.raises(error):
                entry(E(**bad))
        big = E(k=torch.ones((1, 16392), dtype=torch.int32), edges=f64(1, 16392, 1), sigma=f64(1, 16392, 1), misfit=f64(1, 16392))
        with pytest.raises(ValueError, match="16384 slots"):             # refused by name, whatever the chains
            entry(big, chains=8)
        with pytest.raises(_lib.NativeLibraryError):                     # 16 384 slots of four chains are fine
            entry(E(k=torch.ones((1, 16384), dtype=torch.int32), edges=f64(1, 16384, 1), sigma=f64(1, 16384, 1), misfit=f64(1, 16384)), chains=4)
    for kw in (dict(max_lag=0), dict(max_lag=256), dict(block=0), dict(percentiles=(50, 5)), dict(percentiles=())):
        with pytest.raises(ValueError):
            ensembles.rank_diagnostics(E(), edges, **kw)
    with pytest.raises(ValueError):
        ensembles.quantiles(E(), edges, (120,))
    with pytest.raises(ValueError):
        ensembles.quantiles(E(), [3.0, 2.0], (50,))
    with pytest.raises(ValueError):
        ensembles.ensemble_ranks(E(), edges, probabilities=(1.5,))
    # the Python entries on a series
    rows, V = 20, 3
    good = dict(x=f64(B, rows, V), seg_start=torch.tensor([[0, 10], [0, 10]], dtype=torch.int32), seg_m=torch.full((B,), 2, dtype=torch.int32),
                seg_n=torch.full((B,), 10, dtype=torch.int32))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    series = (lambda **kw: ensembles.series_ranks(**dict(good, **kw)), lambda **kw: ensembles.series_rank_diagnostics(**dict(good, **kw)),
              lambda **kw: ensembles.series_correlation(rank=True, **dict(good, **kw)))
    for call in series:
        with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
            call()
        for name in good:
            with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
                call(**{name: good[name].numpy()})
        for kw, error in ((dict(x=f64(B, rows)), ValueError), (dict(x=good["x"].float()), TypeError), (dict(seg_m=good["seg_m"].long()), TypeError),
                          (dict(seg_start=i32([[0, 10], [0, 11]])), ValueError), (dict(seg_m=i32([2, 3])), ValueError),
                          (dict(seg_start=i32([[0, 5], [0, 10]]), seg_n=i32([15, 10])), ValueError),      # 2 x 15 > 20 rows: they overlap
                          (dict(x=f64(1, 16385, 1), seg_start=i32([[0]]), seg_m=i32([1]), seg_n=i32([8])), ValueError)):
            with pytest.raises(error):
                call(**kw)
    with pytest.raises(ValueError, match="16384 rows"):
        ensembles.series_ranks(f64(1, 16385, 1), i32([[0]]), i32([1]), i32([8]))
    for kw in (dict(probabilities=(2.0,)), dict(probabilities=[0.5] * 17)):
        with pytest.raises(ValueError):
            ensembles.series_ranks(**dict(good, **kw))
    for kw in (dict(max_lag=300), dict(percentiles=(95, 5))):
        with pytest.raises(ValueError):
            ensembles.series_rank_diagnostics(**dict(good, **kw))
