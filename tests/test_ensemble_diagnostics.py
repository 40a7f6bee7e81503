"""The rule of the chain diagnostics (geobipy_amd.ensembles.diagnostics_reference: split-chain autocovariances, Geyer's initial
monotone sequence, tau, ESS, split R-hat, MCSE) on the host: hand cases, an independent formulation, AR(1) series with
a known autocorrelation time, chains that disagree, the segment lists, and the refusals every entry makes before the library loads."""
import numpy as np
import pytest

from geobipy_amd import ensembles
from geobipy_amd.ensembles import diagnostics_reference as rule

U = 2.0 ** -52


def _smooth(rng, n_rows, V, scale=0.2):
    """cumsum-smoothed normals, |x| <= 8."""
    return np.clip(np.cumsum(rng.standard_normal((n_rows, V)), axis=0) * scale, -8.0, 8.0)


def test_an_alternating_series_by_hand():
    """x_t = (-1)^t, one segment of N = 8: acov(l) = (-1)^l (N - l) / N, W = N / (N - 1), vp = 1, rho_1 = -N / (N - 1), so P_0 < 0:
    one pair, tau at its floor 1 / log10(N), ess = N log10(N) -- an anticorrelated chain is worth more than its length."""
    N = 8
    x = np.array([(-1.0) ** t for t in range(N)])[:, None] * np.array([[1.0, 3.0]]) + np.array([[0.0, 5.0]])
    r = rule(x, [0], N, 7)
    assert r["L"] == 7 and np.array_equal(r["pairs"], [1, 1])
    assert np.allclose(r["mean"], [0.0, 5.0], rtol=0, atol=4 * U * 8) and np.allclose(r["sd"], [1.0, 3.0], rtol=8 * U)
    want_rho = np.array([1.0] + [1.0 - N / (N - 1.0) * (1.0 - (-1.0) ** l * (N - l) / N) for l in range(1, 8)])
    assert np.allclose(r["rho"][:, 0], want_rho, rtol=0, atol=32 * U) and np.allclose(r["rho"][:, 1], want_rho, rtol=0, atol=32 * U)
    assert np.allclose(r["tau"], 1.0 / np.log10(N), rtol=4 * U) and np.allclose(r["ess"], N * np.log10(N), rtol=8 * U)
    assert np.allclose(r["rhat"], np.sqrt((N - 1.0) / N), rtol=8 * U)              # M = 1: Bn = 0
    assert np.allclose(r["mcse"], r["sd"] / np.sqrt(r["ess"]), rtol=8 * U)


def test_constant_and_non_finite_variables():
    rng = np.random.default_rng(2)
    x = _smooth(rng, 40, 5)
    x[:, 1] = 0.1 + 0.2                                                  # constant: compared as stored, never through a variance
    x[13, 2] = np.nan                                                    # a NaN in a used row
    x[39, 3] = np.inf                                                    # a non-finite value in a row no segment uses
    x[7, 4] = -np.inf
    r = rule(x, [0, 19], 19, 9)
    assert r["mean"][1] == 0.1 + 0.2 and r["sd"][1] == 0.0 and r["pairs"][1] == 0
    assert all(np.isnan(r[n][1]) for n in ("rhat", "tau", "ess", "mcse")) and np.isnan(r["rho"][:, 1]).all()
    for v in (2, 4):
        assert all(np.isnan(r[n][v]) for n in ensembles.STAT_NAMES) and r["pairs"][v] == 0 and np.isnan(r["rho"][:, v]).all()
    for v in (0, 3):
        assert all(np.isfinite(r[n][v]) for n in ensembles.STAT_NAMES) and r["pairs"][v] >= 1 and r["rho"][0, v] == 1.0
    alone = rule(x[:, [0]], [0, 19], 19, 9)
    assert all(np.allclose(alone[n], r[n][[0]], rtol=1e-12, atol=0) for n in ensembles.STAT_NAMES)      # the variables do not see each other


def test_lag_counts_and_short_segments():
    rng = np.random.default_rng(3)
    x = _smooth(rng, 64, 3)
    r = rule(x, [5], 4, 255)                                             # N = 4: L = 3
    assert r["L"] == 3 and np.isfinite(r["rho"][:4]).all() and np.isnan(r["rho"][4:]).all() and r["rho"].shape == (256, 3)
    assert np.all(r["pairs"] >= 1) and np.all(r["pairs"] <= 2)
    for n in (0, 1, 3):                                                  # N < 4: nothing
        r = rule(x, [0, 10], n, 7)
        assert all(np.isnan(r[k]).all() for k in ensembles.STAT_NAMES) and np.all(r["pairs"] == 0) and np.isnan(r["rho"]).all()
    r = rule(x, [], 20, 7)                                               # M = 0: nothing
    assert all(np.isnan(r[k]).all() for k in ensembles.STAT_NAMES) and np.all(r["pairs"] == 0)
    r = rule(x, [0, 30], 30, 6)                                          # an even max_lag: L is lowered, the last lag stays NaN
    assert r["L"] == 5 and np.isfinite(r["rho"][:6]).all() and np.isnan(r["rho"][6]).all() and np.all(r["pairs"] <= 3)
    r = rule(x, [0, 9], 9, 255)                                          # max_lag > N - 1 = 8 (even): L = 7
    assert r["L"] == 7 and np.isfinite(r["rho"][:8]).all() and np.isnan(r["rho"][8:]).all()
    assert int(ensembles.lag_count(9, 255)) == 7 and int(ensembles.lag_count(2048, 255)) == 255 and int(ensembles.lag_count(4, 1)) == 1
    one = rule(x, [0], 60, 15)                                           # M = 1: Bn = 0, rhat = sqrt((N - 1) / N) exactly as computed
    assert np.allclose(one["rhat"], np.sqrt(59.0 / 60.0), rtol=8 * U)
    with pytest.raises(ValueError):
        rule(x, [40], 30, 7)                                             # the segment leaves the rows
    for bad in (0, 256, -1, 2.5, True):
        with pytest.raises(ValueError):
            rule(x, [0], 20, bad)


def _fft_rho(x, starts, N, L):
    """rho by another route: autocovariances from numpy.fft (zero-padded power spectrum), the rule's steps 3 .. 7 on top."""
    M = len(starts)
    n_fft = 1 << int(np.ceil(np.log2(2 * N)))
    acov, means = [], []
    for q in starts:
        seg = x[q:q + N]
        mean = seg.mean(axis=0)
        F = np.fft.rfft(seg - mean, n=n_fft, axis=0)
        acov.append(np.fft.irfft(F * np.conj(F), n=n_fft, axis=0)[:L + 1] / N)
        means.append(mean)
    A = np.mean(acov, axis=0) * N / (N - 1.0)
    means = np.array(means)
    Bn = means.var(axis=0, ddof=1) if M > 1 else 0.0
    vp = A[0] * (N - 1.0) / N + Bn
    rho = 1.0 - (A[0] - A) / vp
    rho[0] = 1.0
    return rho


def _walk(rho):
    P = rho[0::2] + rho[1::2]
    pairs = np.ones(P.shape[1], dtype=np.int32)
    for v in range(P.shape[1]):
        for k in range(1, P.shape[0]):
            if not P[k, v] > 0:
                break
            pairs[v] += 1
    return pairs


def test_the_rule_against_long_double_and_an_fft_formulation():
    """130 rows, 65 variables, M = 2, N = 65, L = 63.  e = max |fp64 rule - long-double rule| of rho (measured: 9.0e-16, the FFT route: 9.0e-16); the FFT route
    agrees with the long-double rule within max(16 e, 16 * 2^-52) and all three walks stop at the same pair."""
    rng = np.random.default_rng(5)
    x = _smooth(rng, 130, 65)
    r64, rld = rule(x, [0, 65], 65, 255), rule(x, [0, 65], 65, 255, dtype=np.longdouble)
    L = r64["L"]
    assert L == 63 and rld["rho"].dtype == np.longdouble
    e = float(np.max(np.abs(r64["rho"][:L + 1] - rld["rho"][:L + 1])))
    bound = max(16 * e, 16 * U)
    rho_fft = _fft_rho(x, [0, 65], 65, L)
    d_fft = float(np.max(np.abs(rho_fft - rld["rho"][:L + 1])))
    print("e = %.3g, fft - long double = %.3g, bound = %.3g, min |P_k| = %.3g" % (e, d_fft, bound, float(np.abs(r64["pair_sums"]).min())))
    assert e <= 64 * U
    assert d_fft <= bound
    assert np.array_equal(r64["pairs"], rld["pairs"]) and np.array_equal(r64["pairs"], _walk(rho_fft)) and np.array_equal(_walk(r64["rho"][:L + 1]), r64["pairs"])
    assert float(np.max(np.abs(r64["tau"] - rld["tau"]))) <= (L + 1) * bound


def _ar1(rng, phi, n, V):
    e = rng.standard_normal((n, V))
    x = np.empty_like(e)
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)                               # the stationary start
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x


def test_ar1_series_give_their_autocorrelation_time():
    """512 independent AR(1) series of 4 096 samples per phi (default_rng(1), phi = 0, 0.5, 0.9 drawn in that order, stationary start),
    split into M = 2 segments of N = 2 048, max_lag 255 (L = 255): the median tau stands within 5 % of (1 + phi) / (1 - phi).
    Measured at L = 255: median +1.6 %, +0.9 %, +0.5 %; mean +2.3 %, +2.0 %, +4.3 % (the estimator's positive bias); cells at the lag
    cap 0, 0, 2 of 512; largest R-hat 1.050."""
    rng = np.random.default_rng(1)
    for phi in (0.0, 0.5, 0.9):
        r = rule(_ar1(rng, phi, 4096, 512), [0, 2048], 2048, 255)
        want = (1.0 + phi) / (1.0 - phi)
        med, mean = float(np.median(r["tau"])) / want - 1.0, float(r["tau"].mean()) / want - 1.0
        print("phi %.1f: median %+.4f mean %+.4f capped %d max rhat %.4f" % (phi, med, mean, int((r["pairs"] == 128).sum()), float(r["rhat"].max())))
        assert abs(med) <= 0.05
        assert np.allclose(r["ess"], 4096.0 / r["tau"], rtol=4 * U) and np.allclose(r["mcse"], r["sd"] / np.sqrt(r["ess"]), rtol=8 * U)
        assert float(r["rhat"].max()) < 1.1 and int((r["pairs"] == 128).sum()) <= 5


def test_chains_that_disagree():
    """Two chains whose means differ by several standard deviations: rhat > 1.1, and the pooled ess falls below that of either chain."""
    rng = np.random.default_rng(7)
    n, V = 400, 16
    a, b = _ar1(rng, 0.5, n, V), _ar1(rng, 0.5, n, V) + 4.0
    x = np.concatenate([a, b])
    N = n // 2
    both = rule(x, [0, N, n, n + N], N, 255)
    one, two = rule(x, [0, N], N, 255), rule(x, [n, n + N], N, 255)
    assert np.all(both["rhat"] > 1.1) and np.all(one["rhat"] < 1.1) and np.all(two["rhat"] < 1.1)
    assert np.all(both["ess"] < np.minimum(one["ess"], two["ess"]))
    assert np.allclose(both["mean"], 0.5 * (one["mean"] + two["mean"]), rtol=0, atol=64 * U) and np.all(both["sd"] > 2.0)
    agree = rule(np.concatenate([a, b - 4.0]), [0, N, n, n + N], N, 255)
    assert np.all(agree["rhat"] < 1.1) and np.all(agree["ess"] > np.maximum(one["ess"], two["ess"]))


def test_segments_from_counts():
    nk = 64
    start, m, n, used = ensembles.segments(np.array([[0], [7], [8], [9], [nk]]), nk)
    assert start.dtype == m.dtype == n.dtype == np.int32 and start.shape == (5, 2)
    assert np.array_equal(m, [0, 0, 2, 2, 2]) and np.array_equal(n, [0, 0, 4, 4, 32]) and np.array_equal(used, [0, 0, 1, 1, 1])
    assert np.array_equal(start[2:], [[0, 4], [0, 4], [0, 32]])          # an odd n = 9: N = 4, slot 8 is not used
    # three chains: an unused replicate in the middle, a short one, the shortest used chain sets n
    start, m, n, used = ensembles.segments(np.array([[nk, 0, nk], [nk, 7, 33], [20, 21, 64], [3, 0, 7]]), nk)
    assert np.array_equal(used, [2, 2, 3, 0]) and np.array_equal(m, [4, 4, 6, 0]) and np.array_equal(n, [32, 16, 10, 0])
    assert np.array_equal(start[0], [0, 32, 128, 160, 0, 0]) and np.array_equal(start[1], [0, 16, 128, 144, 0, 0])
    assert np.array_equal(start[2], [0, 10, 64, 74, 128, 138]) and np.all(start[3] == 0)
    for b in range(3):
        assert np.all(start[b, :m[b]] + n[b] <= 3 * nk) and np.all((start[b, :m[b]] % nk) + n[b] <= nk)       # inside their own chain
    for bad in (dict(count_per_chain=np.array([[65]]), slots_per_chain=64), dict(count_per_chain=np.array([[-1]]), slots_per_chain=64),
                dict(count_per_chain=np.zeros((2, 9), dtype=np.int64), slots_per_chain=64), dict(count_per_chain=np.array([1.5]), slots_per_chain=4),
                dict(count_per_chain=np.array([[1]]), slots_per_chain=0)):
        with pytest.raises(ValueError):
            ensembles.segments(**bad)


def test_refusals_before_the_library_loads(monkeypatch, tmp_path):
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib, survey, survey_run
    from geobipy_amd.__main__ import parse

    def boom():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", boom)
    # the survey driver: the diagnostics need the ensemble; checked before the options are even read
    for kw in (dict(ensemble_diagnostics=True), dict(ensemble_diagnostics=dict(max_lag=7)), dict(ensemble_diagnostics=True, ensemble=False)):
        with pytest.raises(ValueError, match="needs ensemble"):
            survey.infer("no such options file", **kw)
    for bad in (dict(max_lag=0), dict(max_lag=256), dict(max_lag=3.5), dict(lag=3), 7, "yes"):
        with pytest.raises(ValueError):
            survey.infer("no such options file", ensemble=16, ensemble_diagnostics=bad)
    assert survey_run.ensemble_diagnostics_argument(False, None) is None and survey_run.ensemble_diagnostics_argument(None, 16) is None
    assert survey_run.ensemble_diagnostics_argument(True, 16) == dict(max_lag=255)
    assert survey_run.ensemble_diagnostics_argument(dict(max_lag=31), dict(n_keep=8, thin=1)) == dict(max_lag=31)
    # the command line of the survey
    with pytest.raises(SystemExit):
        parse(["options", "out", "--ensemble-diagnostics"])               # without --ensemble
    with pytest.raises(SystemExit):
        parse(["options", "out", "--ensemble", "16", "--ensemble-diagnostics", "256"])
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-diagnostics"]).ensemble_diagnostics == 255
    assert parse(["options", "out", "--ensemble", "16", "--ensemble-diagnostics", "31"]).ensemble_diagnostics == 31
    assert parse(["options", "out", "--ensemble", "16"]).ensemble_diagnostics is None
    # the Python entries: host tensors, shapes, chains, max_lag
    k = torch.ones((2, 12), dtype=torch.int32)
    e, s = torch.full((2, 12, 5), float("inf"), dtype=torch.float64), torch.ones((2, 12, 5), dtype=torch.float64)
    ens = ensembles.Ensemble(k, e, s, torch.ones((2, 12), dtype=torch.float64), (k > 0).sum(dim=1), 3, torch.zeros(2, dtype=torch.float64))
    edges = np.arange(11.0)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        ensembles.diagnostics(ens, edges)
    for kw in (dict(chains=5), dict(chains=0), dict(chains=9), dict(chains=1.5), dict(max_lag=0), dict(max_lag=256), dict(block=0)):
        with pytest.raises(ValueError):
            ensembles.diagnostics(ens, edges, **kw)
    with pytest.raises(ValueError, match="divide"):
        ensembles.diagnostics(ens, edges, chains=5)
    with pytest.raises(ValueError):
        ensembles.diagnostics(ens, [3.0, 2.0])
    x = torch.zeros((2, 20, 3), dtype=torch.float64)
    i32 = lambda *a: torch.zeros(a, dtype=torch.int32)      # noqa: E731
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        ensembles.series_diagnostics(x, i32(2, 2), i32(2), i32(2))
    with pytest.raises(ValueError):
        ensembles.series_diagnostics(x, i32(2, 2), i32(2), i32(2), max_lag=300)
    # the command line of the module
    path, got_edges, chains, max_lag, device = ensembles.parse_args(["run.npz", "--depth-axis", "40", "2.5", "--chains", "2", "--max-lag", "63"])
    assert path == "run.npz" and np.array_equal(got_edges, np.arange(41) * 2.5) and chains == 2 and max_lag == 63 and device == "cuda:0"
    path, got_edges, chains, max_lag, _ = ensembles.parse_args(["run.npz", "--depth-edges", "0", "1", "3", "7"])
    assert np.array_equal(got_edges, [0.0, 1.0, 3.0, 7.0]) and chains == 1 and max_lag == 255
    assert ensembles.diagnostics_path("a/run.npz") == "a/run.diagnostics.npz"
    for bad in (["run.npz"], ["run.npz", "--depth-axis", "40", "2.5", "--depth-edges", "0", "1"], ["run.npz", "--depth-axis", "0", "2.5"],
                ["run.npz", "--depth-axis", "x", "2.5"], ["run.npz", "--depth-edges", "0", "2", "1"], ["run.npz", "--depth-edges", "0"],
                ["run.npz", "--depth-axis", "4", "1", "--max-lag", "0"], ["run.npz", "--depth-axis", "4", "1", "--chains", "9"],
                ["--depth-axis", "4", "1"]):
        with pytest.raises(SystemExit):
            ensembles.parse_args(bad)


def test_python_entries_refuse_bad_shapes_dtypes_and_segments(monkeypatch):
    """Shapes, dtypes and the segment lists are refused before the device is asked for, so host tensors reach every check: these
    checks are what keeps the kernel inside seg_start / seg_m / seg_n and inside the rows they name."""
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib

    def boom():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", boom)
    B, rows, V = 2, 20, 3
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)      # noqa: E731
    good = dict(x=f64(B, rows, V), seg_start=torch.tensor([[0, 10], [0, 10]], dtype=torch.int32), seg_m=torch.full((B,), 2, dtype=torch.int32),
                seg_n=torch.full((B,), 10, dtype=torch.int32))
    call = lambda **kw: ensembles.series_diagnostics(**dict(good, **kw))      # noqa: E731
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        call()                                                           # all in order, but on the host
    for name in good:                                                    # numpy arrays and lists are no device tensors
        with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
            call(**{name: good[name].numpy()})
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    for kw, error in ((dict(x=f64(B, rows)), ValueError), (dict(x=f64(B, rows, V, 1)), ValueError), (dict(x=f64(B, 0, V)), ValueError),
                      (dict(x=f64(B, rows, 0)), ValueError), (dict(x=f64(1, 32769, 1), seg_start=i32([[0]]), seg_m=i32([1]), seg_n=i32([8])), ValueError),
                      (dict(x=good["x"].float()), TypeError), (dict(x=good["x"].long()), TypeError),
                      (dict(seg_start=good["seg_start"].long()), TypeError), (dict(seg_m=good["seg_m"].long()), TypeError),
                      (dict(seg_n=good["seg_n"].double()), TypeError),
                      (dict(seg_start=i32([0, 10])), ValueError),                                  # not [B, M_max]
                      (dict(seg_start=i32([[0, 10]])), ValueError),                                # another B
                      (dict(seg_start=torch.zeros((B, 0), dtype=torch.int32)), ValueError),        # M_max = 0
                      (dict(seg_start=torch.zeros((B, 17), dtype=torch.int32)), ValueError),       # M_max = 17
                      (dict(seg_m=i32([2, 2, 2])), ValueError), (dict(seg_m=i32([[2], [2]])), ValueError),
                      (dict(seg_n=i32([10])), ValueError), (dict(seg_n=i32([[10, 10]])), ValueError),
                      (dict(seg_m=i32([2, 3])), ValueError),                                       # more segments than seg_start has columns
                      (dict(seg_m=i32([2, -1])), ValueError), (dict(seg_n=i32([10, -4])), ValueError),
                      (dict(seg_start=i32([[0, 10], [0, 11]])), ValueError),                       # 11 + 10 > 20 rows
                      (dict(seg_start=i32([[-1, 10], [0, 10]])), ValueError),
                      (dict(seg_n=i32([10, 21])), ValueError)):
        with pytest.raises(error):
            call(**kw)
    with pytest.raises(_lib.NativeLibraryError):                         # a start outside the rows in a column no segment uses is fine
        call(seg_start=i32([[0, 10], [0, 99]]), seg_m=i32([2, 1]))
    # the ensemble entry
    ns, K = 12, 5
    ens = dict(k=torch.ones((B, ns), dtype=torch.int32), edges=torch.full((B, ns, K), float("inf"), dtype=torch.float64), sigma=f64(B, ns, K) + 1.0,
               misfit=f64(B, ns) + 1.0, count=torch.full((B,), ns), thin=3, log_mean_prior=f64(B))
    diag = lambda chains=1, **kw: ensembles.diagnostics(ensembles.Ensemble(**dict(ens, **kw)), np.arange(11.0), chains=chains)      # noqa: E731
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        diag()
    for name in ("k", "edges", "sigma", "misfit"):
        with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
            diag(**{name: ens[name].numpy()})
    for kw, error in ((dict(k=ens["k"][0]), ValueError), (dict(edges=ens["edges"][:, :, 0]), ValueError), (dict(sigma=f64(B, ns, K + 1)), ValueError),
                      (dict(k=torch.ones((B, ns + 1), dtype=torch.int32)), ValueError), (dict(k=torch.ones((B + 1, ns), dtype=torch.int32)), ValueError),
                      (dict(misfit=f64(B, ns + 1)), ValueError), (dict(misfit=f64(B)), ValueError),
                      (dict(k=ens["k"].long()), TypeError), (dict(edges=ens["edges"].float()), TypeError), (dict(sigma=ens["sigma"].float()), TypeError),
                      (dict(misfit=ens["misfit"].long()), TypeError),
                      (dict(edges=f64(B, ns, 65), sigma=f64(B, ns, 65)), ValueError),                                         # K = 65
                      (dict(edges=f64(B, ns, 0), sigma=f64(B, ns, 0)), ValueError),                                           # K = 0
                      (dict(k=torch.ones((1, 4097), dtype=torch.int32), edges=f64(1, 4097, 1), sigma=f64(1, 4097, 1), misfit=f64(1, 4097)), ValueError)):
        with pytest.raises(error):
            diag(**kw)
    with pytest.raises(_lib.NativeLibraryError):                         # 8 192 slots are fine for two chains
        diag(chains=2, k=torch.ones((1, 8192), dtype=torch.int32), edges=f64(1, 8192, 1), sigma=f64(1, 8192, 1), misfit=f64(1, 8192))
