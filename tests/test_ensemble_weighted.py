"""Weighted per-column products: the rule on the host (geobipy_amd.ensembles weighted_reference, quantise_weights).

``weighted_reference`` is held to brute force -- every value written out q times and the type-1 quantile and the counts of that
expanded sample taken -- on tiny columns; the refusals come by message; the planted line of test_sections.py shows what the weights are
for: where a sounding's posterior holds a decoy family of 10 of its 16 models, the equal-weight median sits on the decoy and the
median under the chain's smoothed marginals on the true family."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, ensembles, sections
from test_sections import Z1_LINE, planted_line

ONE = 2 ** 40


def _brute(values, q, probabilities, thresholds):
    """Type-1 quantiles and counts >= a threshold of the sample that holds values[u] q[u] times (None: it is empty)."""
    sample = np.sort(np.repeat(values, q))
    if sample.size == 0:
        return None
    quantile = [sample[max(math.ceil(p * sample.size), 1) - 1] for p in probabilities]
    return quantile, [int((sample >= t).sum()) for t in thresholds], sample.mean(), sample.std()


def test_reference_against_the_expanded_sample():
    rng = np.random.default_rng(11)
    probs, thr = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0), (-1.0, 0.0, 0.5)
    levels = np.array([-1.0, -0.5, 0.0, 0.5, 2.0])                    # five levels: ties abound; 0.0 and 0.5 are thresholds too
    cases = 0
    for m in range(1, 7):
        for _ in range(40):
            n_rows, V = 9, 3
            x = rng.choice(levels, (1, n_rows, V))
            rows = rng.permutation(n_rows)[:6].astype(np.int32)[None, :]
            q = rng.integers(0, 6, (1, 6)).astype(np.int64)
            out = ensembles.weighted_reference(x, rows, np.array([m]), q, probs, thr)
            for v in range(V):
                want = _brute(x[0, rows[0, :m], v], q[0, :m], probs, thr)
                if want is None:
                    assert out["total"][0] == 0 and np.isnan(out["quantile"][0, :, v]).all() and np.all(out["above"][0, :, v] == 0)
                    assert np.isnan(out["mean"][0, v]) and np.isnan(out["sd"][0, v])
                    continue
                assert out["total"][0] == q[0, :m].sum()
                assert np.array_equal(out["quantile"][0, :, v], want[0]) and np.array_equal(out["above"][0, :, v], want[1])
                assert abs(out["mean"][0, v] - want[2]) <= 1e-14 and abs(out["sd"][0, v] - want[3]) <= 1e-14
                cases += 1
    assert cases > 500


def test_reference_edge_cases():
    x = np.array([[[3.0], [1.0], [np.nan], [1.0], [2.0], [np.inf]]])          # [1, 6, 1]
    rows = np.array([[0, 1, 2, 3, 4, 5]], dtype=np.int32)
    probs = (0.0, 0.5, 1.0)
    # a q = 0 row takes no part whatever it holds (NaN, +inf) or names (-7, 99); the rows past n_used neither
    q = np.array([[1, 2, 0, 2, 5, 0]], dtype=np.int64)
    out = ensembles.weighted_reference(x, rows, np.array([6]), q, probs, (1.0, 2.5))
    assert out["total"][0] == 10 and out["quantile"][0, :, 0].tolist() == [1.0, 2.0, 3.0] and out["above"][0, :, 0].tolist() == [10, 1]
    wild = rows.copy()
    wild[0, 2], wild[0, 5] = -7, 99
    again = ensembles.weighted_reference(x, wild, np.array([6]), q, probs, (1.0, 2.5))
    assert all(np.array_equal(out[name], again[name], equal_nan=True) for name in out)
    short = ensembles.weighted_reference(x, rows, np.array([2]), np.array([[1, 2, 7, 7, 7, 7]], dtype=np.int64), probs, (1.0, 2.5))
    assert short["total"][0] == 3 and short["quantile"][0, :, 0].tolist() == [1.0, 1.0, 3.0] and short["above"][0, :, 0].tolist() == [3, 1]
    # ties: C jumps by the summed weight of the run; p = 0.4 of W = 10 is reached by the two 1.0 (weight 4) exactly
    assert ensembles.weighted_reference(x, rows, np.array([6]), q, (0.4, 0.41), None)["quantile"][0, :, 0].tolist() == [1.0, 2.0]
    # W = 0: n_used = 0, or all q 0
    for nu, qq in ((0, q), (6, np.zeros_like(q))):
        z = ensembles.weighted_reference(x, rows, np.array([nu]), qq, probs, (1.0,))
        assert z["total"][0] == 0 and np.isnan(z["quantile"]).all() and np.all(z["above"] == 0) and np.isnan(z["mean"]).all() and np.isnan(z["sd"]).all()
    # a non-finite participating value: the column is NaN, above -1; the other column is not touched
    x2 = np.concatenate([x, np.arange(6.0).reshape(1, 6, 1)], axis=2)
    for bad in (2, 5):
        qb = q.copy()
        qb[0, bad] = 1
        z = ensembles.weighted_reference(x2, rows, np.array([6]), qb, probs, (1.0,))
        assert np.isnan(z["quantile"][0, :, 0]).all() and z["above"][0, 0, 0] == -1 and np.isnan(z["mean"][0, 0]) and np.isnan(z["sd"][0, 0])
        assert np.isfinite(z["quantile"][0, :, 1]).all() and z["above"][0, 0, 1] == qb[0, 1:].sum() and z["total"][0] == 11
    # q outside 0 .. 2^40 is clamped
    c = ensembles.weighted_reference(x, rows, np.array([2]), np.array([[-5, 2 ** 45, 0, 0, 0, 0]], dtype=np.int64), probs, None)
    assert c["total"][0] == ONE and c["quantile"][0, :, 0].tolist() == [1.0, 1.0, 1.0]
    # long double moments
    ld = ensembles.weighted_reference(x, rows, np.array([6]), q, None, None, dtype=np.longdouble)
    assert ld["mean"].dtype == np.longdouble and abs(float(ld["mean"][0, 0]) - 1.7) < 1e-15


@pytest.mark.parametrize("n", [1, 2, 7, 20, 64])
def test_equal_weights_give_the_type_1_order_statistic(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=(1, n, 2))
    rows = np.arange(n, dtype=np.int32)[None, :]
    probs = np.array([0.0, 0.05, 0.3, 0.5, 0.95, 1.0])
    for weight in (1, 3, ONE):
        out = ensembles.weighted_reference(x, rows, np.array([n]), np.full((1, n), weight, dtype=np.int64), probs, None)
        for v in range(2):
            s = np.sort(x[0, :, v])
            assert out["quantile"][0, :, v].tolist() == [s[max(math.ceil(p * n), 1) - 1] for p in probs]
    if n >= 20:                                                        # NOT the interpolated quantile of ensembles.quantiles
        assert out["quantile"][0, 2, 0] != np.quantile(x[0, :, 0], 0.3)


def test_quantise_weights():
    w = np.array([[0.25, 1.0, 0.5, 7.0], [0.0, 0.0, 0.0, 0.0], [3.0, 2.0 ** -42 * 3.0, 1.0, np.nan], [np.nan, -1.0, np.inf, 5.0]])
    nu = np.array([3, 4, 3, 0])
    q = ensembles.quantise_weights(w, nu)
    assert q.dtype == np.int64 and q.tolist() == [[ONE // 4, ONE, ONE // 2, 0], [0, 0, 0, 0], [ONE, 0, round(ONE / 3), 0], [0, 0, 0, 0]]
    assert q[2, 2] == np.rint(1.0 / 3.0 * 2.0 ** 40)                   # one division, one exact scaling, rint
    t = ensembles.quantise_weights(torch.as_tensor(w), torch.as_tensor(nu))
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), q)
    assert np.array_equal(ensembles.quantise_weights(torch.as_tensor(w).float(), nu.astype(np.int32)).numpy(), ensembles.quantise_weights(w.astype(np.float32), nu))
    rng = np.random.default_rng(5)
    big = rng.uniform(size=(7, 300)) ** 8
    nb = rng.integers(0, 301, 7)
    qb = ensembles.quantise_weights(big, nb)
    assert np.array_equal(ensembles.quantise_weights(torch.as_tensor(big), nb).numpy(), qb)
    for b in range(7):
        assert np.all(qb[b, nb[b]:] == 0) and (nb[b] == 0 or qb[b, :nb[b]].max() == ONE) and qb[b].sum() <= 2 ** 52
    for conv in (np.asarray, torch.as_tensor):
        for bad in (np.nan, -1e-300, np.inf):
            ww = w[:1].copy()
            ww[0, 1] = bad
            with pytest.raises(ValueError, match="NaN, infinite or negative"):
                ensembles.quantise_weights(conv(ww), np.array([3]))
        with pytest.raises(ValueError, match="floating point"):
            ensembles.quantise_weights(conv(np.ones((2, 2), dtype=np.int64)), np.array([1, 1]))
        with pytest.raises(ValueError, match="floating point"):
            ensembles.quantise_weights(conv(np.ones(3)), np.array([1]))
        for bad_nu in (np.array([1]), np.array([1.0, 1.0]), np.array([1, 5]), np.array([-1, 1])):
            with pytest.raises(ValueError, match="n_used"):
                ensembles.quantise_weights(conv(np.ones((2, 4))), bad_nu)


def _host_ensemble(S=2, ns=8, K=4):
    k = torch.ones((S, ns), dtype=torch.int32)
    e = torch.full((S, ns, K), float("inf"), dtype=torch.float64)
    s = torch.ones((S, ns, K), dtype=torch.float64)
    return ensembles.Ensemble(k, e, s, None, None, 1, None)


def test_refusals_come_before_the_library():
    x = np.zeros((2, 5, 3))
    rows, nu, q = np.zeros((2, 4), dtype=np.int32), np.array([4, 4]), np.ones((2, 4), dtype=np.int64)
    for bad, match in (((x[0], rows, nu, q), "x \\[B, n_rows, V\\]"), ((x, rows[0], nu, q), "rows"), ((x, rows.astype(np.float64), nu, q), "rows"),
                       ((x, np.zeros((2, 4097), dtype=np.int32), nu, np.ones((2, 4097), dtype=np.int64)), "rows"), ((x, rows, nu, q[:, :3]), "q holds"),
                       ((x, rows, nu, q.astype(np.float64)), "q holds"), ((x, rows, nu[:1], q), "q holds")):
        with pytest.raises(ValueError, match=match):
            ensembles.weighted_reference(*bad)
    for probs in ([-0.1], [1.5], [np.nan], np.zeros(17)):
        with pytest.raises(ValueError, match="probabilities"):
            ensembles.weighted_reference(x, rows, nu, q, probs)
    for thr in ([np.nan], [np.inf], np.zeros(9), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="thresholds"):
            ensembles.weighted_reference(x, rows, nu, q, None, thr)

    tx, trows, tnu, tq = torch.as_tensor(x), torch.as_tensor(rows), torch.as_tensor(nu, dtype=torch.int32), torch.as_tensor(q)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        ensembles.series_weighted(x, trows, tnu, tq)
    with pytest.raises(TypeError, match="float64"):
        ensembles.series_weighted(tx.float(), trows, tnu, tq)
    with pytest.raises(ValueError, match="n_rows"):
        ensembles.series_weighted(tx[0], trows, tnu, tq)
    for bad in ((trows[0], tnu, tq), (trows[:1], tnu, tq), (trows, tnu[:1], tq), (trows, tnu, tq[:, :2])):
        with pytest.raises(ValueError, match="rows|n_used"):
            ensembles.series_weighted(tx, *bad)
    for bad in ((trows.long(), tnu, tq), (trows, tnu.long(), tq), (trows, tnu, tq.int()), (trows, tnu, tq.double())):
        with pytest.raises(TypeError, match="int32"):
            ensembles.series_weighted(tx, *bad)
    with pytest.raises(ValueError, match="percentiles"):
        ensembles.series_weighted(tx, trows, tnu, tq, percentiles=(50, 5))
    with pytest.raises(ValueError, match="thresholds"):
        ensembles.series_weighted(tx, trows, tnu, tq, thresholds=[np.nan])
    with pytest.raises(_lib.NativeLibraryError, match="gbp_series_weighted"):
        ensembles.series_weighted(tx, trows, tnu, tq)

    ens, edges = _host_ensemble(), np.arange(0.0, 11.0)
    w = torch.ones((2, 4), dtype=torch.float64)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        ensembles.weighted(ens, edges, rows, w)
    for kw, err, match in ((dict(depth_edges=[0.0]), ValueError, "depth_edges"), (dict(percentiles=()), ValueError, "percentiles"),
                           (dict(percentiles=(101,)), ValueError, "percentiles"), (dict(thresholds=np.zeros(9)), ValueError, "thresholds"),
                           (dict(block=0), ValueError, "block"), (dict(weight=w.float()), TypeError, "float64 .* or int64"),
                           (dict(weight=w[:, :3]), ValueError, "q \\[B, n\\]"), (dict(rows=trows[:1]), ValueError, "rows"),
                           (dict(rows=trows.long()), TypeError, "int32"), (dict(n_used=tnu[:1]), ValueError, "n_used"),
                           (dict(n_used=tnu.long()), TypeError, "int32"), (dict(weight=-w), ValueError, "negative"),
                           (dict(weight=w * float("nan")), ValueError, "NaN"), (dict(ens=ens._replace(k=ens.k[:, :3])), ValueError, "ensemble"),
                           (dict(ens=ens._replace(sigma=ens.sigma.float())), TypeError, "ensemble")):
        args = dict(dict(ens=ens, depth_edges=edges, rows=trows, weight=w, n_used=tnu), **kw)
        with pytest.raises(err, match=match):
            ensembles.weighted(**args)
    for weight in (w, tq):
        with pytest.raises(_lib.NativeLibraryError, match="gbp_ensemble_weighted"):
            ensembles.weighted(ens, edges, trows, weight)

    s = dict(rows=trows, n_used=tnu, weight=w)
    with pytest.raises(ValueError, match="holds no weight"):
        sections.lateral_products(ens, dict(rows=trows, n_used=tnu), edges)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_ensemble_weighted"):
        sections.lateral_products(ens, s, edges)
    xy = np.zeros(2)
    for products in ([0.0, 1.0], dict(percentiles=(50,)), dict(depth_edges=edges, depth=3), dict(depth_edges=[1.0]), dict(depth_edges=edges, percentiles=(50, 5)),
                     dict(depth_edges=edges, thresholds=[np.inf])):
        with pytest.raises(ValueError, match="products|depth_edges|percentiles|thresholds"):
            sections.sections(ens, xy, xy, 10.0, products=products)
    with pytest.raises(ValueError, match="marginals=True"):
        sections.sections(ens, xy, xy, 10.0, marginals=False, products=dict(depth_edges=edges))
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.sections(ens, xy, xy, 10.0, products=dict(depth_edges=edges))


def test_the_command_line(capsys):
    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--depth-axis", "120", "1", "--percentiles", "10", "50", "90", "--exceed", "-1", "-0.5"])
    assert path == "run.npz" and set(kw["products"]) == {"depth_edges", "percentiles", "thresholds"}
    assert np.array_equal(kw["products"]["depth_edges"], np.arange(121.0)) and kw["products"]["percentiles"] == (10.0, 50.0, 90.0)
    assert kw["products"]["thresholds"] == (-1.0, -0.5)
    _, kw = sections.parse_args(["run.npz", "--depth", "150", "--depth-axis", "60", "2.5"])
    assert kw["products"]["percentiles"] == (5.0, 50.0, 95.0) and kw["products"]["thresholds"] == () and kw["products"]["depth_edges"][-1] == 150.0
    assert "products" not in sections.parse_args(["run.npz", "--depth", "150"])[1]
    for extra in (["--percentiles", "50"], ["--exceed", "0"], ["--depth-axis", "0", "1"], ["--depth-axis", "x", "1"], ["--depth-axis", "10", "-1"],
                  ["--depth-axis", "10", "1", "--no-marginals"], ["--depth-axis", "10", "1", "--percentiles", "50", "5"],
                  ["--depth-axis", "10", "1", "--exceed"] + ["0"] * 9):
        with pytest.raises(SystemExit):
            sections.parse_args(["run.npz", "--depth", "150"] + extra)
    capsys.readouterr()


def test_signatures_declare_both_entries():
    assert len(_lib.SIGNATURES["gbp_series_weighted"][1]) == 17 and len(_lib.SIGNATURES["gbp_ensemble_weighted"][1]) == 21


# ---- the planted line ---------------------------------------------------------------------------------------------------------------

DEPTH_EDGES_LINE = np.arange(0.0, Z1_LINE + 1.0)                     # a 1 m axis from 0 to 120 m


def planted_cells(k, edges, sigma):
    """The (sounding, cell) pairs of the planted line the weights decide: every sounding with a decoy family (its first 10 models) and
    every cell centre more than 4 m inside the gap between the mean first interfaces of the two families.  Returns (s, cell, the true
    family's mean log10 value there, the decoy family's), arrays, computed from the models alone."""
    z = ensembles.centres(DEPTH_EDGES_LINE)
    x = np.log10(ensembles.realisations_reference(k, edges, sigma, DEPTH_EDGES_LINE))      # [S, n, n_depth]
    out = []
    for s in range(k.shape[0]):
        top = edges[s, :, 0]
        lo, hi = sorted((top[:10].mean(), top[10:].mean()))
        if hi - lo <= 10.0:                                            # no decoy: the families are 15 m apart, the jitter is 1 m
            continue
        for c in np.nonzero((z > lo + 4.0) & (z < hi - 4.0))[0]:
            out.append((s, c, x[s, 10:, c].mean(), x[s, :10, c].mean()))
    return tuple(np.array(a) for a in zip(*out))


def check_planted_products(median_equal, median_weighted, k, edges, sigma):
    """The property of the planted line, given the equal-weight and the weighted median [S, n_depth]: in every cell of ``planted_cells``
    the two families' values differ by more than 1 decade, the equal-weight median is within 0.3 of the decoy family's value and the
    weighted median within 0.3 of the true family's; at least 50 such cells exist."""
    s, c, true_value, decoy_value = planted_cells(k, edges, sigma)
    print("planted line: %d cells in %d decoy soundings" % (s.size, np.unique(s).size))
    assert s.size >= 50
    assert np.all(np.abs(true_value - decoy_value) > 1.0)
    print("equal weights: at most %.3f from the decoy; weighted: at most %.3f from the truth"
          % (np.abs(median_equal[s, c] - decoy_value).max(), np.abs(median_weighted[s, c] - true_value).max()))
    assert np.all(np.abs(median_equal[s, c] - decoy_value) < 0.3)
    assert np.all(np.abs(median_weighted[s, c] - true_value) < 0.3)


def test_the_planted_line_on_the_rules_alone():
    k, edges, sigma, x, y, truth = planted_line()
    S, n = k.shape
    rows = np.tile(np.arange(n, dtype=np.int32), (S, 1))
    n_used = np.full(S, n, dtype=np.int32)
    d2 = sections.cross_distance_reference(k, edges, sigma, rows, sections.partners(None, n_used), 0.0, Z1_LINE)
    weight = sections.track_reference([0, S], None, sections.steps(x, y), d2, n_used)["marginal"]
    values = np.log10(ensembles.realisations_reference(k, edges, sigma, DEPTH_EDGES_LINE))
    equal = ensembles.weighted_reference(values, rows, n_used, np.ones((S, n), dtype=np.int64), [0.5])
    q = ensembles.quantise_weights(weight, n_used)
    assert q.max(axis=1).tolist() == [ONE] * S
    lateral = ensembles.weighted_reference(values, rows, n_used, q, [0.5])
    check_planted_products(equal["quantile"][:, 0], lateral["quantile"][:, 0], k, edges, sigma)
