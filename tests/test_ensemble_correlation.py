"""The rule of the correlation between depth cells (geobipy_amd.ensembles.correlation_reference: pooled sample covariance and
correlation in a band; correlation_runs_reference / resolution_length: the runs above a threshold) on the host: numpy's
own estimators, the long-double evaluation, hand cases, and the refusals every entry makes before the library loads."""
import numpy as np
import pytest

from geobipy_amd import ensembles
from geobipy_amd.ensembles import correlation_reference as rule
from geobipy_amd.ensembles import correlation_runs_reference as runs

U = 2.0 ** -52


def _smooth(rng, n_rows, V, scale=0.2):
    """cumsum-smoothed normals across the variables too, so neighbours correlate; |x| <= 8."""
    x = np.cumsum(rng.standard_normal((n_rows, V)), axis=0) * scale
    return np.clip(x + 0.5 * np.roll(x, 1, axis=1), -8.0, 8.0)


def _full(x, starts, n, **kw):
    return rule(x, starts, n, x.shape[1] - 1, **kw)


def test_the_rule_against_numpy_on_segments_with_gaps():
    rng = np.random.default_rng(1)
    x = _smooth(rng, 60, 9)
    starts, n = [3, 20, 41], 13                                          # rows 0 - 2, 16 - 19, 33 - 40, 54 - 59 are not used
    used = np.concatenate([x[q:q + n] for q in starts])
    got = _full(x, starts, n)
    assert got["band"].shape == (9, 9) and got["mean"].shape == (9,) and got["sd"].shape == (9,)
    assert np.allclose(got["mean"], used.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(got["sd"], used.std(axis=0, ddof=1), rtol=1e-12, atol=0)
    R = ensembles.band_to_matrix(got["band"])
    assert np.allclose(R, np.corrcoef(used, rowvar=False), rtol=0, atol=1e-12)
    C = ensembles.band_to_matrix(_full(x, starts, n, normalise=False)["band"])
    assert np.allclose(C, np.cov(used, rowvar=False, ddof=1), rtol=0, atol=1e-12)
    assert np.all(np.diag(R) == 1.0)                                     # written, not computed
    # the unused rows do not enter: overwrite them with anything
    y = x.copy()
    mask = np.ones(60, dtype=bool)
    for q in starts:
        mask[q:q + n] = False
    y[mask] = np.nan
    again = _full(y, starts, n)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)


def test_the_fp64_rule_against_its_long_double_evaluation():
    rng = np.random.default_rng(2)
    x = _smooth(rng, 300, 20)
    starts, n = [0, 150], 150
    a, b = rule(x, starts, n, 11), rule(x, starts, n, 11, dtype=np.longdouble)
    assert b["band"].dtype == np.longdouble and a["band"].dtype == np.float64
    sd = b["sd"].astype(np.float64)
    eps = 8 * (300 + 8) * U * (1 + np.abs(x).max() / sd.min())
    assert np.array_equal(np.isnan(a["band"]), np.isnan(b["band"].astype(np.float64)))
    ok = ~np.isnan(a["band"])
    assert np.max(np.abs(a["band"][ok] - b["band"][ok])) <= eps
    assert np.max(np.abs(a["mean"] - b["mean"])) <= eps * np.abs(x).max() and np.max(np.abs(a["sd"] - b["sd"]) / b["sd"]) <= eps


def test_constant_non_finite_and_linear_columns():
    rng = np.random.default_rng(3)
    x = _smooth(rng, 40, 7)
    base = _full(x, [0, 20], 20)
    y = x.copy()
    y[:, 2] = 0.1 + 0.2                                                  # a constant
    y[7, 4] = np.nan                                                     # a NaN in a used row
    y[:, 5] = -3.0 * y[:, 1] + 0.5                                       # exact linear relations
    y[:, 6] = 2.0 * y[:, 1] - 1.0
    got = _full(y, [0, 20], 20)
    assert got["mean"][2] == 0.1 + 0.2 and got["sd"][2] == 0.0 and np.isnan(got["mean"][4]) and np.isnan(got["sd"][4])
    R, R0 = ensembles.band_to_matrix(got["band"]), ensembles.band_to_matrix(base["band"])
    dead = np.zeros(7, dtype=bool)
    dead[[2, 4]] = True
    assert np.isnan(R[dead]).all() and np.isnan(R[:, dead]).all()        # every entry that involves them, their diagonals included
    keep = np.ix_([0, 1, 3], [0, 1, 3])
    assert np.array_equal(R[keep], R0[keep])                             # no other entry is touched
    assert abs(R[1, 5] + 1.0) <= 1e-14 and abs(R[1, 6] - 1.0) <= 1e-14 and abs(R[5, 6] + 1.0) <= 1e-14
    inf = x.copy()
    inf[3, 0] = np.inf
    assert np.isnan(_full(inf, [0, 20], 20)["band"][0]).all() and np.isnan(_full(inf, [0, 20], 20)["mean"][0])
    # a NaN in an unused row changes nothing
    z = x.copy()
    z[39, 3] = np.nan
    short = _full(z, [0, 20], 19)
    assert all(np.array_equal(short[k], _full(x, [0, 20], 19)[k], equal_nan=True) for k in short) and np.isfinite(short["band"][3, 0])


def test_short_and_empty_soundings_and_the_band():
    rng = np.random.default_rng(4)
    x = _smooth(rng, 12, 5)
    for starts, n in (([], 6), ([0], 3), ([0, 4, 8], 1)):                # M = 0; n = 3; three segments of one row
        got = rule(x, starts, n, 2)
        assert all(np.isnan(got[k]).all() for k in got) and got["band"].shape == (5, 3)
    four = rule(x, [0, 6], 2, 2)                                         # n = 4 is enough
    assert np.isfinite(four["sd"]).all()
    full, cut = rule(x, [0], 12, 4), rule(x, [0], 12, 2)
    assert np.array_equal(cut["band"], full["band"][:, :3], equal_nan=True)
    for c in range(5):                                                   # the NaN tail c + j >= V, nothing else
        assert np.array_equal(np.isnan(full["band"][c]), c + np.arange(5) >= 5)
    zero = rule(x, [0], 12, 0)
    assert zero["band"].shape == (5, 1) and np.all(zero["band"] == 1.0)
    one = rule(x[:, :1], [0], 12, 0)
    assert one["band"].shape == (1, 1) and one["band"][0, 0] == 1.0
    for bad in (-1, 5, 2.5, True):
        with pytest.raises(ValueError):
            rule(x, [0], 12, bad)
    with pytest.raises(ValueError):
        rule(x, [7], 6, 2)                                               # leaves the rows
    with pytest.raises(ValueError):
        rule(x[0], [0], 12, 0)
    # sd is the pooled one: O(1 / N) from the diagnostics' sqrt(vp) for segments that agree (white noise: their means differ by
    # O(sd / sqrt(N)), which enters the two variances with weights that differ by O(1))
    y = rng.standard_normal((400, 3))
    d = ensembles.diagnostics_reference(y, [0, 200], 200, 15)
    assert np.allclose(_full(y, [0, 200], 200)["sd"], d["sd"], rtol=8.0 / 200, atol=0)


def test_band_to_matrix_round_trip():
    rng = np.random.default_rng(5)
    V, W = 6, 2
    band = rng.uniform(-1, 1, (3, V, W + 1))
    for c in range(V):
        band[:, c, max(0, V - c):] = np.nan
    m = ensembles.band_to_matrix(band)
    assert m.shape == (3, V, V) and np.array_equal(m, np.swapaxes(m, 1, 2), equal_nan=True)
    for c in range(V):
        for v in range(V):
            j = abs(v - c)
            assert np.array_equal(m[:, c, v], band[:, min(c, v), j], equal_nan=True) if j <= W else np.isnan(m[:, c, v]).all()
    back = np.stack([np.concatenate([np.diagonal(m, j, 1, 2), np.full((3, j), np.nan)], axis=1) for j in range(W + 1)], axis=2)
    assert np.array_equal(back, band, equal_nan=True)
    torch = pytest.importorskip("torch")
    assert np.array_equal(ensembles.band_to_matrix(torch.as_tensor(band)).numpy(), m, equal_nan=True)
    assert np.array_equal(ensembles.band_to_matrix(band[0]), m[0], equal_nan=True)
    with pytest.raises(ValueError):
        ensembles.band_to_matrix(np.zeros((3, 4)))                       # W + 1 > V


def _band(V, W, value=1.0):
    b = np.full((V, W + 1), value)
    for c in range(V):
        b[c, V - c:] = np.nan
    return b


def test_runs_and_resolution_length_by_hand():
    edges = np.array([0.0, 1.0, 3.0, 6.0, 10.0, 15.0, 21.0])
    V = 6
    ones = runs(_band(V, 2), 0.5)                                        # all ones: every walk ends at j = W or at the axis' end
    assert np.array_equal(ones["down"], [2, 2, 2, 2, 1, 0]) and np.array_equal(ones["up"], [0, 1, 2, 2, 2, 2])
    assert not ones["closed_up"].any() and not ones["closed_down"].any()
    length = ensembles.resolution_length(ones["up"], ones["down"], edges)
    assert np.array_equal(length, [6.0, 10.0, 15.0, 20.0, 18.0, 15.0]) and np.all(length >= np.diff(edges))
    b = _band(V, 3)
    b[2, 0] = np.nan                                                     # cell 2 is dead: every entry that involves it is NaN
    b[2, 1:] = np.nan
    b[1, 1] = b[0, 2] = np.nan
    r = runs(b, 0.5)
    assert r["up"][2] == r["down"][2] == 0 and not r["closed_up"][2] and not r["closed_down"][2]
    assert r["down"][1] == 0 and r["closed_down"][1] and r["up"][3] == 0 and r["closed_up"][3]       # a NaN neighbour closes the run
    assert r["down"][0] == 1 and r["closed_down"][0] and r["up"][1] == 1 and not r["closed_up"][1]
    assert r["down"][3] == 2 and not r["closed_down"][3]                 # ... 3, 4, 5: the end of the axis
    live = ~np.isnan(b[:, 0])
    length = ensembles.resolution_length(r["up"], r["down"], edges, live=live)
    assert np.isnan(length[2]) and np.array_equal(length[[0, 1, 3]], [3.0, 3.0, 15.0])
    t = _band(V, 2, 0.75)                                                # a threshold hit exactly counts (>=)
    at, above = runs(t, 0.75), runs(t, np.nextafter(0.75, 1.0))
    assert np.array_equal(at["down"], ones["down"]) and not at["closed_down"].any()
    assert not above["down"].any() and not above["up"].any()
    assert np.array_equal(above["closed_down"], [True] * 5 + [False]) and np.array_equal(above["closed_up"], [False] + [True] * 5)
    w0 = runs(_band(V, 0), 0.5)                                          # W = 0: nothing to walk, nothing closed
    assert not w0["up"].any() and not w0["down"].any() and not w0["closed_up"].any() and not w0["closed_down"].any()
    assert np.array_equal(ensembles.resolution_length(w0["up"], w0["down"], edges), np.diff(edges))
    assert w0["up"].dtype == np.int32 and w0["closed_up"].dtype == bool
    torch = pytest.importorskip("torch")
    tl = ensembles.resolution_length(torch.as_tensor(r["up"]), torch.as_tensor(r["down"]), edges, live=torch.as_tensor(live))
    assert np.array_equal(tl.numpy(), length, equal_nan=True)
    with pytest.raises(ValueError):
        runs(np.zeros((2, 3)), 0.5)
    with pytest.raises(ValueError):
        ensembles.resolution_length(r["up"], r["down"], edges[:-1])


def test_refusals_before_the_library_loads(monkeypatch):
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib, survey, survey_run
    from geobipy_amd.__main__ import parse

    def boom():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", boom)
    # the survey driver: the correlation needs the ensemble; checked before the options are even read
    for kw in (dict(ensemble_correlation=True), dict(ensemble_correlation=dict(band=7)), dict(ensemble_correlation=True, ensemble=False)):
        with pytest.raises(ValueError, match="needs ensemble"):
            survey.infer("no such options file", **kw)
    for bad in (dict(band=-1), dict(band=3.5), dict(band=True), dict(threshold=0.0), dict(threshold=1.0), dict(threshold="x"), dict(keep_band=1),
                dict(width=3), 7, "yes"):
        with pytest.raises(ValueError):
            survey.infer("no such options file", ensemble=16, ensemble_correlation=bad)
    arg = survey_run.ensemble_correlation_argument
    assert arg(False, None) is None and arg(None, 16) is None
    assert arg(True, 16) == dict(band=64, threshold=0.5, keep_band=False)
    assert arg(dict(band=0, threshold=0.9, keep_band=True), dict(n_keep=8, thin=1)) == dict(band=0, threshold=0.9, keep_band=True)
    # the command line of the survey
    for bad in (["options", "out", "--ensemble-correlation"], ["options", "out", "--ensemble", "16", "--ensemble-correlation", "-1"],
                ["options", "out", "--ensemble", "16", "--ensemble-correlation", "8", "1.0"],
                ["options", "out", "--ensemble", "16", "--ensemble-correlation", "8", "0"],
                ["options", "out", "--ensemble", "16", "--ensemble-correlation", "x"],
                ["options", "out", "--ensemble", "16", "--ensemble-correlation", "8", "0.5", "3"]):
        with pytest.raises(SystemExit):
            parse(bad)
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-correlation"]).ensemble_correlation == dict(band=64, threshold=0.5)
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-correlation", "0", "0.25"]).ensemble_correlation == dict(band=0, threshold=0.25)
    assert parse(["options", "out", "--ensemble", "16"]).ensemble_correlation is None
    # the command line of the module
    assert ensembles.parse_correlation(["run.npz", "--depth-axis", "40", "2.5"]) is None
    assert ensembles.parse_correlation(["run.npz", "--depth-axis", "40", "2.5", "--correlation"]) == (64, 0.5)
    assert ensembles.parse_correlation(["run.npz", "--depth-axis", "40", "2.5", "--correlation", "9", "--threshold", "0.8", "--chains", "2"]) == (9, 0.8)
    assert ensembles.parse_args(["run.npz", "--depth-axis", "40", "2.5", "--correlation", "9", "--chains", "2"])[2] == 2
    assert ensembles.correlation_path("a/run.npz") == "a/run.correlation.npz"
    for bad in (["run.npz", "--depth-axis", "4", "1", "--correlation", "-1"], ["run.npz", "--depth-axis", "4", "1", "--correlation", "x"],
                ["run.npz", "--depth-axis", "4", "1", "--correlation", "--threshold", "1"],
                ["run.npz", "--depth-axis", "4", "1", "--correlation", "--threshold", "0"],
                ["run.npz", "--depth-axis", "4", "1", "--threshold", "0.5"],
                ["run.npz", "--depth-axis", "4", "1", "--correlation", "--max-lag", "7"]):
        with pytest.raises(SystemExit):
            ensembles.parse_correlation(bad)
    with pytest.raises(SystemExit):
        ensembles.main(["run.npz", "--depth-axis", "4", "1", "--correlation", "--chains", "9"])
    # the Python entries: every shape, dtype and value check comes before the device is asked for
    B, ns, K = 2, 12, 5
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)      # noqa: E731
    ens = dict(k=torch.ones((B, ns), dtype=torch.int32), edges=torch.full((B, ns, K), float("inf"), dtype=torch.float64), sigma=f64(B, ns, K) + 1.0,
               misfit=f64(B, ns) + 1.0, count=torch.full((B,), ns), thin=3, log_mean_prior=f64(B))
    edges = np.arange(11.0)
    corr = lambda e=edges, **kw: ensembles.correlation(ensembles.Ensemble(**dict(ens, **{k: v for k, v in kw.items() if k in ens})), e,      # noqa: E731
                                                       **{k: v for k, v in kw.items() if k not in ens})
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        corr()
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        corr(band=1000, keep_band=False)                                 # the band is clipped to n_depth - 1
    for name in ("k", "edges", "sigma"):
        with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
            corr(**{name: ens[name].numpy()})
    for kw in (dict(chains=5), dict(chains=0), dict(chains=9), dict(chains=1.5), dict(band=-1), dict(band=2.0), dict(band=True), dict(threshold=0.0),
               dict(threshold=1.0), dict(threshold=None), dict(block=0), dict(block=1.5), dict(e=[3.0, 2.0]), dict(k=ens["k"][0]),
               dict(edges=ens["edges"][:, :, 0]), dict(sigma=f64(B, ns, K + 1)), dict(k=torch.ones((B + 1, ns), dtype=torch.int32)),
               dict(edges=f64(B, ns, 65), sigma=f64(B, ns, 65)), dict(edges=f64(B, ns, 0), sigma=f64(B, ns, 0)),
               dict(k=torch.ones((1, 4097), dtype=torch.int32), edges=f64(1, 4097, 1), sigma=f64(1, 4097, 1))):
        with pytest.raises(ValueError):
            corr(**kw)
    for kw in (dict(k=ens["k"].long()), dict(edges=ens["edges"].float()), dict(sigma=ens["sigma"].float())):
        with pytest.raises(TypeError):
            corr(**kw)
    good = dict(x=f64(B, 20, 3), seg_start=torch.tensor([[0, 10], [0, 10]], dtype=torch.int32), seg_m=torch.full((B,), 2, dtype=torch.int32),
                seg_n=torch.full((B,), 10, dtype=torch.int32))
    call = lambda **kw: ensembles.series_correlation(**dict(good, **kw))      # noqa: E731
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        call()
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        call(band=99, normalise=False)
    for name in good:
        with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
            call(**{name: good[name].numpy()})
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    for kw, error in ((dict(x=f64(B, 20)), ValueError), (dict(x=f64(B, 0, 3)), ValueError), (dict(x=f64(B, 20, 0)), ValueError),
                      (dict(x=f64(1, 32769, 1), seg_start=i32([[0]]), seg_m=i32([1]), seg_n=i32([8])), ValueError),
                      (dict(x=good["x"].float()), TypeError), (dict(seg_start=good["seg_start"].long()), TypeError),
                      (dict(band=-1), ValueError), (dict(band=1.0), ValueError),
                      (dict(seg_start=torch.zeros((B, 17), dtype=torch.int32)), ValueError), (dict(seg_m=i32([2, 3])), ValueError),
                      (dict(seg_start=i32([[0, 10], [0, 11]])), ValueError), (dict(seg_n=i32([10, 21])), ValueError)):
        with pytest.raises(error):
            call(**kw)
    band = f64(B, 6, 3)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        ensembles.correlation_runs(band, 0.5)
    with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
        ensembles.correlation_runs(band.numpy(), 0.5)
    for b, t, error in ((band.float(), 0.5, TypeError), (band[0], 0.5, ValueError), (f64(B, 2, 3), 0.5, ValueError), (band, float("nan"), ValueError)):
        with pytest.raises(error):
            ensembles.correlation_runs(b, t)
