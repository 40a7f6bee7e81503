"""Local mixture fits and global classes (geobipy_amd/mixtures.py, hitmap.mixture, csrc/gbp_hitmap.h k_hitmap_mixture).
The reference fits its mixtures with one lmfit optimisation per column, whose path cannot be reproduced: the rule is stated on the host
(mixtures.mixture_reference) and held (i) to scikit-learn's GaussianMixture on the expanded sample from the same initial values and to
its closed forms -- CPU tier, with ``select`` against a plain loop, the refusals and the command lines --, and (ii) on the GPU the kernel
is held to the statement on every column of small planted blocks and of the committed hit maps, and ``from_results`` / the command lines
end to end on the committed line container.

Measured (the figures the tests print):
  host rule against scikit-learn 1.7.2, 90 fits at 40 iterations: largest difference in weight / mean / variance 1.4e-12 (bar 1e-9);
  kernel against the host rule on an MI355X, every column of the planted blocks and of the committed maps, Kmax 1 .. 4, 1 / 7 / 50
  iterations, int32 and int64: weight 4.3e-15, mean 9.2e-15, sd 1.0e-14, ll_change 1.8e-15 (absolute); loglik 1.2e-12, misfit 4.1e-13
  (relative) -- DEVICE_BAR below is 10 x these."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from geobipy_amd import mixtures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAPS = os.path.join(HERE, "golden", "line_products.npz")
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")

# The kernel against the host rule: 10 x the worst difference measured on the blocks below and on the committed maps (the header), never
# looser than 1e-9 -- absolute for weight, mean, sd and ll_change (a difference of two log-likelihoods), relative for the misfits and
# the log-likelihood.
DEVICE_BAR = dict(weight=4.3e-14, mean=9.2e-14, sd=1.1e-13, ll_change=1.8e-14, loglik=1.2e-11, misfit=4.1e-12)
assert max(DEVICE_BAR.values()) <= 1e-9


def _start(c, x, K, reg):
    """The rule's initial values for one column, written out from its statement."""
    N = int(c.sum())
    m = float((c * x).sum() / N)
    V = float((c * (x - m) ** 2).sum() / N)
    cum = np.cumsum(c.astype(np.int64))
    mu = np.array([x[int(np.argmax(2 * K * cum >= (2 * j + 1) * N))] for j in range(K)])
    return np.full(K, 1.0 / K), mu, np.full(K, V / K ** 2 + reg)


def _populations(rng, nv, N, n_pop, W):
    """A histogram [nv] of N draws from 1 .. 3 well-separated normal populations on the axis of half-width W."""
    centres = np.array([[0.0], [-0.9, 0.8], [-1.3, 0.0, 1.2]][n_pop - 1]) * W / 2.0 + rng.uniform(-0.05, 0.05, n_pop)
    which = rng.integers(0, n_pop, N)
    s = centres[which] + rng.normal(0.0, 0.09 * W / 2.0, N)
    return np.histogram(np.clip(s, -W + 1e-9, W - 1e-9), bins=nv, range=(-W, W))[0].astype(np.int64)


# -- the host rule -------------------------------------------------------------------------------------------------------------------

def test_rule_is_scikit_learns_em_on_the_expanded_sample():
    sk = pytest.importorskip("sklearn.mixture")
    import warnings
    rng = np.random.default_rng(4)
    nv, N, W, n_iter = 64, 3000, 2.0, 40
    x = mixtures.centres(nv, W)
    reg = (2.0 * W / nv) ** 2 / 12.0
    cols = [_populations(rng, nv, N, n_pop, W) for n_pop in (1, 2, 3) for _ in range(10)]
    ref = mixtures.mixture_reference(np.stack(cols, axis=1)[None], W, max_components=3, n_iter=n_iter)
    worst = 0.0
    for i, c in enumerate(cols):
        sample = np.repeat(x, c)[:, None]
        for K in (1, 2, 3):
            w0, mu0, s0 = _start(c.astype(np.float64), x, K, reg)
            g = sk.GaussianMixture(K, covariance_type="spherical", tol=0.0, max_iter=n_iter, reg_covar=reg, weights_init=w0,
                                   means_init=mu0[:, None], precisions_init=1.0 / s0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                g.fit(sample)
            s = K * (K - 1) // 2
            d = max(np.abs(ref["weight"][0, s:s + K, i] - g.weights_).max(), np.abs(ref["mean"][0, s:s + K, i] - g.means_[:, 0]).max(),
                    np.abs(ref["sd"][0, s:s + K, i] ** 2 - g.covariances_).max())
            worst = max(worst, d)
    print("host rule against scikit-learn: largest difference", worst)
    assert worst <= 1e-9


def test_closed_forms():
    W, nv = 1.5, 16
    x = mixtures.centres(nv, W)
    reg = (2.0 * W / nv) ** 2 / 12.0
    rng = np.random.default_rng(2)
    h = np.zeros((1, nv, 6), dtype=np.int64)
    h[0, :, 0] = rng.integers(0, 50, nv)                             # a general column
    h[0, 5, 1] = 9                                                   # a single cell
    h[0, 2, 2] = h[0, 13, 2] = 40                                    # two equal cells far apart
    h[0, :, 3] = 7 * h[0, :, 0]                                      # the general column x 7
    h[0, 0, 4] = 3                                                   # mass only in the first cell ...
    h[0, nv - 1, 5] = 3                                              # ... and only in the last
    r = mixtures.mixture_reference(h, W, max_components=4, n_iter=30)
    assert all(np.isfinite(v).all() for v in r.values())             # fewer non-empty cells than components: still finite
    c = h[0, :, 0].astype(np.float64)
    m = (c * x).sum() / c.sum()
    V = (c * (x - m) ** 2).sum() / c.sum()
    assert abs(r["weight"][0, 0, 0] - 1.0) == 0.0 and abs(r["mean"][0, 0, 0] - m) <= 1e-12 and abs(r["sd"][0, 0, 0] ** 2 - (V + reg)) <= 1e-12
    assert r["ll_change"][0, 0, 0] == 0.0
    for col, v in ((1, 5), (4, 0), (5, nv - 1)):                     # a single cell: every component sits on it with variance reg
        assert np.abs(r["mean"][0, :, col] - x[v]).max() <= 1e-12 and np.abs(r["sd"][0, :, col] ** 2 - reg).max() <= 1e-12
        for K in (1, 2, 3, 4):
            s = K * (K - 1) // 2
            assert abs(r["weight"][0, s:s + K, col].sum() - 1.0) <= 1e-12
    assert np.abs(r["mean"][0, 1:3, 2] - [x[2], x[13]]).max() <= 1e-12 and np.abs(r["weight"][0, 1:3, 2] - 0.5).max() <= 1e-12
    assert np.abs(r["sd"][0, 1:3, 2] ** 2 - reg).max() <= 1e-12
    for k in ("weight", "mean", "sd", "misfit", "loglik"):           # counts x 7: the same fit
        assert np.abs(r[k][..., 3] - r[k][..., 0]).max() <= 1e-12, k
    # other arguments: one iteration, an explicit reg, K = 1 alone
    one = mixtures.mixture_reference(h, W, max_components=1, n_iter=1, reg=0.01)
    assert one["weight"].shape == (1, 1, 6) and abs(one["sd"][0, 0, 0] ** 2 - (V + 0.01)) <= 1e-12
    for bad in (dict(max_components=0), dict(max_components=5), dict(n_iter=0), dict(n_iter=10001), dict(reg=0.0), dict(reg=float("nan"))):
        with pytest.raises(ValueError):
            mixtures.mixture_reference(h, W, **bad)


def test_empty_columns_and_maps_give_nan_and_no_components():
    h = np.zeros((2, 8, 3), dtype=np.int32)
    h[0, 3, 1] = 4
    r = mixtures.mixture_reference(h, 1.0, max_components=3, n_iter=5)
    for k, v in r.items():
        assert np.isnan(v[1]).all() and np.isnan(v[0][..., 0]).all() and np.isfinite(v[0][..., 1]).all(), k
    s = mixtures.select(r, log_mean_prior=np.array([-2.0, -3.0]))
    assert s["n_components"].dtype == torch.int32 and s["n_components"].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert torch.isnan(s["mean"][1]).all() and torch.isnan(s["misfit"][0, :, 0]).all() and torch.isnan(s["loglik"][1]).all()
    assert abs(float(s["mean"][0, 0, 1]) - (mixtures.centres(8, 1.0)[3] - 2.0 / np.log(10.0))) <= 1e-15
    assert torch.isnan(s["mean"][0, 1:, 1]).all() and torch.isnan(s["weight"][0, 1:, 1]).all()
    e = mixtures.mixture_reference(np.zeros((0, 8, 3), dtype=np.int32), 1.0)
    assert e["weight"].shape == (0, 6, 3) and e["misfit"].shape == (0, 3, 2, 3)
    assert mixtures.select(e)["n_components"].shape == (0, 3)


# -- select --------------------------------------------------------------------------------------------------------------------------

def _select_loop(misfit, epsilon=0.05, mu=0.1):
    """The stopping rule as a plain loop over the columns of misfit [B, Kmax, 2, nz] (numpy): the number of components."""
    B, Kmax, _, nz = misfit.shape
    out = np.zeros((B, nz), dtype=np.int32)
    for b in range(B):
        for z in range(nz):
            f = misfit[b, :, :, z]
            if np.isnan(f[0]).any():
                continue
            n = 1
            while n < Kmax:
                if not (f[n - 1, 0] > epsilon and f[n - 1, 1] > epsilon):
                    break
                better = f[n, 1] < f[n - 1, 1]
                moved = abs(f[n, 0] - f[n - 1, 0]) > mu or abs(f[n, 1] - f[n - 1, 1]) > mu
                if not (better and moved):
                    break
                n += 1
            out[b, z] = n
    return out


def _stages_from_misfits(cols):
    """Stages (torch) whose misfits are ``cols`` [(inf_1, two_1), (inf_2, two_2), ...] per column and whose components are numbered."""
    Kmax = len(cols[0])
    mf = torch.tensor(cols, dtype=torch.float64).permute(1, 2, 0)[None].contiguous()      # [1, Kmax, 2, nz]
    nz, S = len(cols), Kmax * (Kmax + 1) // 2
    slot = torch.arange(S, dtype=torch.float64)[None, :, None].expand(1, S, nz)
    per = torch.arange(Kmax, dtype=torch.float64)[None, :, None].expand(1, Kmax, nz)
    return dict(weight=slot + 0.25, mean=-slot, sd=slot + 0.5, loglik=per + 10.0, ll_change=per + 20.0, misfit=mf)


def test_select_is_the_stopping_rule():
    nan = float("nan")
    cols = [
        [(0.04, 0.5), (0.01, 0.1), (0.0, 0.0), (0.0, 0.0)],          # the epsilon stop: the max-norm misfit is small enough
        [(0.5, 0.05), (0.01, 0.01), (0.0, 0.0), (0.0, 0.0)],         # ... the 2-norm misfit is (0.05 does not exceed epsilon)
        [(0.5, 0.5), (0.2, 0.5), (0.0, 0.0), (0.0, 0.0)],            # no decrease of the 2-norm (equal)
        [(0.5, 0.5), (0.1, 0.6), (0.0, 0.0), (0.0, 0.0)],            # an increase
        [(0.5, 0.5), (0.45, 0.45), (0.0, 0.0), (0.0, 0.0)],          # a decrease, but both change by less than mu
        [(0.5, 0.5), (0.04, 0.39), (0.01, 0.2), (0.0, 0.0)],         # accepted once (the 2-norm moved by more than mu), then epsilon
        [(0.5, 0.5), (0.3, 0.45), (0.29, 0.44), (0.0, 0.0)],         # accepted through the max-norm alone, then too small a step
        [(0.9, 0.9), (0.7, 0.7), (0.5, 0.5), (0.3, 0.3)],            # accepted up to Kmax
        [(0.9, 0.9), (0.7, 0.7), (0.5, 0.5), (0.3, 0.6)],            # ... but for the last
        [(nan, nan), (nan, nan), (nan, nan), (nan, nan)],            # an empty column
        [(0.9, 0.9), (nan, nan), (0.1, 0.1), (0.0, 0.0)],            # a NaN further on stops the walk
        [(0.9, 0.9), (0.7, 0.8 - 0.1), (0.0, 0.0), (0.0, 0.0)],      # a step of mu within rounding: as the loop decides
    ]
    st = _stages_from_misfits(cols)
    want = _select_loop(st["misfit"].numpy())
    assert want[0].tolist()[:11] == [1, 1, 1, 1, 1, 2, 2, 4, 3, 0, 1]
    s = mixtures.select(st)
    assert s["n_components"].dtype == torch.int32 and np.array_equal(s["n_components"].numpy(), want)
    for z, n in enumerate(want[0]):
        base = n * (n - 1) // 2
        # means are minus the slot number: sorted ascending, the chosen stage's slots come out in reverse
        assert s["mean"][0, :n, z].tolist() == [-(base + n - 1 - j) for j in range(n)] and torch.isnan(s["mean"][0, n:, z]).all()
        assert s["weight"][0, :n, z].tolist() == [base + n - 1 - j + 0.25 for j in range(n)] and torch.isnan(s["sd"][0, n:, z]).all()
        if n:
            assert float(s["loglik"][0, z]) == 10.0 + n - 1 and float(s["ll_change"][0, z]) == 20.0 + n - 1
            assert s["misfit"][0, :, z].tolist() == list(cols[z][n - 1])
    # other thresholds, and Kmax = 1
    for eps, mu in ((0.0, 0.0), (0.6, 0.1), (0.05, 0.3)):
        assert np.array_equal(mixtures.select(st, eps, mu)["n_components"].numpy(), _select_loop(st["misfit"].numpy(), eps, mu))
    one = _stages_from_misfits([[(0.5, 0.5)], [(nan, nan)]])
    assert mixtures.select(one)["n_components"].tolist() == [[1, 0]]
    # random misfits
    rng = np.random.default_rng(0)
    mf = rng.uniform(0.0, 1.0, size=(3, 4, 2, 50)) * rng.choice([0.1, 1.0], size=(3, 4, 2, 50))
    mf[1, :, :, 7] = np.nan
    st = dict(weight=np.zeros((3, 10, 50)), mean=rng.normal(size=(3, 10, 50)), sd=np.ones((3, 10, 50)), loglik=np.zeros((3, 4, 50)),
              ll_change=np.zeros((3, 4, 50)), misfit=mf)
    s = mixtures.select(st)
    assert np.array_equal(s["n_components"].numpy(), _select_loop(mf))
    m = s["mean"].numpy()
    assert np.all((np.diff(m, axis=1) >= 0) | np.isnan(np.diff(m, axis=1)))


# -- refusals and parsing ------------------------------------------------------------------------------------------------------------

def test_python_entry_refuses_host_tensors_and_bad_arguments():
    from geobipy_amd import _lib, hitmap
    ok = torch.ones((2, 4, 5), dtype=torch.int32)
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.mixture(ok, 1.0)                                      # a host tensor: no fallback
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.mixture(ok.to(torch.int64), 1.0, max_components=4, n_iter=1, reg=0.5)
    with pytest.raises(_lib.NativeLibraryError):
        mixtures.fit(ok, torch.zeros(2, dtype=torch.float64), 1.0)
    for bad in (ok.to(torch.float64), ok.to(torch.int16)):
        with pytest.raises(TypeError):
            hitmap.mixture(bad, 1.0)
    with pytest.raises(ValueError):
        hitmap.mixture(ok.transpose(1, 2), 1.0)                      # not contiguous
    with pytest.raises(TypeError):
        hitmap.mixture(ok[0], 1.0)
    for kw in (dict(max_components=0), dict(max_components=5), dict(n_iter=0), dict(n_iter=10001), dict(reg=0.0), dict(reg=-1.0),
               dict(reg=float("inf")), dict(reg=float("nan"))):
        with pytest.raises(ValueError):
            hitmap.mixture(ok, 1.0, **kw)
    with pytest.raises(ValueError):
        hitmap.mixture(ok, 0.0)


@pytest.mark.parametrize("name", ["gbp_hitmap_mixture", "gbp_hitmap_mixture_i64"])
def test_c_abi_refuses_bad_arguments(name):
    import re
    from geobipy_amd import _lib
    lib = _lib.load()                                               # (a library that does not load is a failure, not a skip)
    assert name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "geobipy_amd.h")).read()
    assert name in set(re.findall(r"\b(gbp_[a-z0-9_]+)\s*\(", hdr))
    entry = getattr(lib, name)
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, nv=250, nz=440, hm=p, Kmax=3, n_iter=50, reg=1e-4, weight=p, mean=p, sd=p, loglik=p, ll_change=p, misfit=p):
        return entry(B, nv, nz, hm, 2.3, Kmax, n_iter, reg, weight, mean, sd, loglik, ll_change, misfit, None)

    none = dict(hm=None, weight=None, mean=None, sd=None, loglik=None, ll_change=None, misfit=None)
    assert call(B=0, **none) == 0                                   # an empty block: no launch
    assert call(B=0, Kmax=5, **none) == INVALID                     # (checked before B == 0)
    assert call(B=-1) == INVALID and call(nv=0) == INVALID and call(nz=0) == INVALID and call(nz=-2) == INVALID
    assert call(nv=4097) == INVALID and b"4096" in lib.gbp_last_error()
    assert call(Kmax=0) == INVALID and call(Kmax=5) == INVALID and call(Kmax=-1) == INVALID
    assert call(n_iter=0) == INVALID and call(n_iter=10001) == INVALID and call(n_iter=-4) == INVALID
    for reg in (0.0, -1e-3, float("inf"), float("nan")):
        assert call(reg=reg) == INVALID, reg
    for k in none:
        assert call(**{k: None}) == INVALID, k
    assert call(B=1 << 30, nz=4) == INVALID and b"range" in lib.gbp_last_error()
    assert call(nz=256 * 65536) == INVALID and b"range" in lib.gbp_last_error()
    assert b"gbp_hitmap_mixture" in lib.gbp_last_error()


def test_command_lines_parse_their_arguments():
    from geobipy_amd import line_products as lp
    a = lp.parse_args(["x.h5"])
    assert a.mixtures is None
    assert lp.parse_args(["x.h5", "--mixtures"]).mixtures == dict(max_components=3, n_iter=50)
    assert lp.parse_args(["x.h5", "--mixtures", "4", "--mixture-iterations", "20"]).mixtures == dict(max_components=4, n_iter=20)
    a = lp.parse_args(["x.h5", "--mixtures", "1", "--depth-intervals", "0", "10"])
    assert a.mixtures["max_components"] == 1 and a.intervals["kind"] == "depth"
    for tail in (["--mixtures", "0"], ["--mixtures", "5"], ["--mixtures", "two"], ["--mixture-iterations", "20"],
                 ["--mixtures", "--mixture-iterations", "0"], ["--mixtures", "--mixture-iterations", "10001"]):
        with pytest.raises(SystemExit):
            lp.parse_args(["x.h5"] + tail)
    assert lp.check_mixtures(True, 250, 2.3)["max_components"] == 3
    got = lp.check_mixtures(dict(max_components=2, mu=0.2), 250, 2.5)
    assert got == dict(max_components=2, n_iter=50, reg=0.02 ** 2 / 12.0, epsilon=0.05, mu=0.2)
    for bad in (dict(components=2), dict(max_components=7), dict(epsilon=-1.0), dict(n_iter=0)):
        with pytest.raises(ValueError):
            lp.check_mixtures(bad, 250, 2.3)
    m = mixtures.parse_args(["lines", "a.products.npz", "--classes", "3"])
    assert m.paths == ["lines", "a.products.npz"] and m.classes == 3 and m.bins == 512 and m.out is None
    assert mixtures.parse_args(["d", "--classes", "16", "--bins", "64", "--out", "c.npz"]).bins == 64
    for tail in ([], ["--classes", "0"], ["--classes", "17"], ["--classes", "2", "--bins", "1"], ["--classes", "2", "--iterations", "0"]):
        with pytest.raises(SystemExit):
            mixtures.parse_args(["d"] + tail)


# -- global classes ------------------------------------------------------------------------------------------------------------------

def _hand_made_fit(rng, clusters, shape=(4, 3, 40)):
    """A fit whose finite local means scatter tightly about ``clusters``; the rest is NaN."""
    which = rng.integers(0, len(clusters), size=shape)
    mean = np.asarray(clusters)[which] + rng.normal(0.0, 0.02, size=shape)
    mean[rng.random(shape) < 0.3] = np.nan
    return dict(mean=torch.as_tensor(mean))


def test_global_classes_on_hand_made_fits(tmp_path):
    from geobipy_amd import line_products as lp
    rng = np.random.default_rng(8)
    for clusters in ([-2.5, -0.5], [-3.0, -1.6, -0.2]):
        fits = [_hand_made_fit(rng, clusters) for _ in range(3)]
        g = mixtures.global_classes(fits, len(clusters), bins=256)
        mu, sd = lp.check_classes(g["means"], g["scales"])
        assert np.all(np.diff(mu) > 0) and np.abs(mu - clusters).max() < 0.02 and np.all(sd < 0.05) and abs(g["weights"].sum() - 1.0) < 1e-12
        n_finite = sum(int(torch.isfinite(f["mean"]).sum()) for f in fits)
        assert g["histogram"].dtype == np.int64 and g["histogram"].sum() == n_finite and g["edges"].size == 257
        one = mixtures.global_classes(fits[0], len(clusters), bins=256)       # one fit, not a list
        assert np.abs(one["means"] - clusters).max() < 0.03
    # the products' name for the means serves too; a single value; nothing finite
    g1 = mixtures.global_classes(dict(mixture_mean=np.full((2, 2, 3), -1.25), mean=np.zeros((2, 3))), 1)      # (a line's products)
    assert abs(g1["means"][0] + 1.25) <= 1.0 / 512 and g1["scales"][0] > 0.0       # (a unit range about the value: within a cell)
    with pytest.raises(ValueError):
        mixtures.global_classes(dict(mean=torch.full((2, 2, 3), float("nan"))), 2)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            mixtures.global_classes(fits, bad)
    # the command line on products files
    for i, f in enumerate(fits):
        np.savez(str(tmp_path / ("%d.0.products.npz" % i)), mixture_mean=f["mean"].numpy(), mean=np.zeros(3))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.mixtures", str(tmp_path), "--classes", "3", "--bins", "256"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    z = dict(np.load(str(tmp_path / "global_classes.npz")))
    want = mixtures.global_classes(fits, 3, bins=256)
    assert set(z) == {"means", "scales", "weights", "histogram", "edges"}
    for k in z:
        assert np.array_equal(z[k], want[k]), k
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("--class-means")][0].split()
    a = lp.parse_args(["x.h5"] + line)
    assert np.allclose(a.class_means, want["means"], rtol=1e-5) and np.allclose(a.class_scales, want["scales"], rtol=1e-5)
    np.savez(str(tmp_path / "9.0.products.npz"), mean=np.zeros(3))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.mixtures", str(tmp_path / "9.0.products.npz"), "--classes", "2"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "mixture_mean" in r.stderr


# -- the kernel against the host rule ------------------------------------------------------------------------------------------------

SHAPES = [(3, 37, 70), (2, 250, 257), (1, 8, 1), (2, 64, 64)]


def _planted(shape, wide):
    """Narrow random columns with N from 1 to 1e5 and the corner cases planted; ``wide``: int64 with counts beyond 2^31."""
    B, nv, nz = shape
    rng = np.random.default_rng(B * 1000 + nv + nz + (7 if wide else 0))
    v = np.arange(nv)[None, :, None]
    h = np.zeros(shape, dtype=np.int64)
    for _ in range(2):                                               # one or two populations per column
        centre = rng.uniform(0.0, nv, size=(B, 1, nz))
        width = rng.uniform(0.4, max(0.5, nv / 12.0), size=(B, 1, nz))
        on = rng.random((B, 1, nz)) < 0.7
        N = 10.0 ** rng.uniform(0.0, 5.0, size=(B, 1, nz))
        h += np.where(on, np.floor(N * np.exp(-0.5 * ((v - centre) / width) ** 2) / (2.5 * width)), 0.0).astype(np.int64)
    z = lambda i: min(i, nz - 1)                                     # noqa: E731
    if nz > 1:
        h[0, :, z(0)] = 0                                            # an empty column
        h[0, :, z(1)] = 0
        h[0, nv // 2, z(1)] = 1                                      # a single cell, N = 1
        h[0, :, z(2)] = 0
        h[0, 0, z(2)] = 100000                                       # mass only in the first value cell ...
        h[0, :, z(3)] = 0
        h[0, nv - 1, z(3)] = 17                                      # ... only in the last
        h[0, :, z(4)] = 0
        h[0, 1, z(4)] = h[0, nv - 2, z(4)] = 50                      # two cells as far apart as they go
        h[0, :, z(5)] = 0
        h[0, :min(nv, 3), z(5)] = [5, 9, 2][:min(nv, 3)]             # fewer non-empty cells than components
    if nz > 40:
        h[0, :, 30:40] = 0
        h[0, 2, 30:40] = 30                                          # a wave whose lanes sit at the bottom of the axis ...
        h[0, :, 35] = 0
        h[0, nv - 3:, 35] = [4, 20, 6]                               # ... but for one at the top: its span is far from its neighbours'
    if B > 1:
        h[B - 1] = 0                                                 # an empty sounding ...
        h[B - 1, nv // 3, nz // 2] = 12                              # ... but for one column
    if not wide:
        return h.astype(np.int32)
    h[0] *= 1 << 22                                                  # counts beyond 2^31 (below 2^53 in every column)
    assert h.max() > 1 << 31 and h.sum(axis=1).max() < 1 << 52
    return h


@functools.lru_cache(maxsize=None)
def _reference(shape, wide, n_iter):
    """The block, and the host rule on it at Kmax = 4 (the stages of a smaller Kmax are its first)."""
    h = _planted(shape, wide)
    return h, mixtures.mixture_reference(h, 2.3, max_components=4, n_iter=n_iter)


def _hold_stages_to(got, ref, Kmax, tag):
    """Every column of the kernel's stages against the host rule's first Kmax stages; returns the largest differences."""
    S = Kmax * (Kmax + 1) // 2
    worst = {}
    for k, rel in (("weight", False), ("mean", False), ("sd", False), ("ll_change", False), ("loglik", True), ("misfit", True)):
        g = got[k].cpu().numpy()
        r = ref[k][:, :S] if k in ("weight", "mean", "sd") else ref[k][:, :Kmax]
        assert g.shape == r.shape, (tag, k, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k)
        assert not np.isinf(g).any(), (tag, k)
        f = ~np.isnan(r)
        d = np.abs(g[f] - r[f]) / (np.maximum(np.abs(r[f]), np.finfo(np.float64).tiny) if rel else 1.0)
        worst[k] = float(d.max()) if d.size else 0.0
    print(tag, " ".join("%s %.2e" % kv for kv in worst.items()))
    for k, d in worst.items():
        assert d <= DEVICE_BAR[k], (tag, k, d)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("n_iter", [1, 7, 50])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_host_rule(shape, n_iter, wide):
    from geobipy_amd import hitmap
    h, ref = _reference(shape, wide, n_iter)
    if shape[2] > 40:                                                # the planted cases are what they were planted as
        assert np.isnan(ref["mean"][0, :, 0]).all() and np.isfinite(ref["mean"][0, :, 1]).all() and np.isfinite(ref["mean"][0, :, 35]).all()
        assert np.isnan(ref["mean"][-1]).sum() == ref["mean"][-1].size - ref["mean"].shape[1]
    d = torch.as_tensor(h).cuda()
    assert d.dtype == (torch.int64 if wide else torch.int32)
    for Kmax in (1, 2, 3, 4):
        got = hitmap.mixture(d, 2.3, max_components=Kmax, n_iter=n_iter)
        _hold_stages_to(got, ref, Kmax, "%s %s Kmax %d n_iter %d" % (shape, "int64" if wide else "int32", Kmax, n_iter))


@pytest.mark.gpu
def test_kernel_takes_an_explicit_reg_and_an_empty_block():
    from geobipy_amd import hitmap
    h = _planted((2, 64, 64), False)
    ref = mixtures.mixture_reference(h, 1.1, max_components=2, n_iter=9, reg=0.003)
    _hold_stages_to(hitmap.mixture(torch.as_tensor(h).cuda(), 1.1, max_components=2, n_iter=9, reg=0.003), ref, 2, "reg 0.003")
    e = hitmap.mixture(torch.zeros((0, 64, 64), dtype=torch.int32).cuda(), 1.1)
    assert e["weight"].shape == (0, 6, 64) and e["misfit"].shape == (0, 3, 2, 64)
    f = mixtures.fit(torch.zeros((0, 64, 64), dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float64).cuda(), 1.1)
    assert f["n_components"].shape == (0, 64) and f["mean"].shape == (0, 3, 64)


def _fixture():
    m = dict(np.load(MAPS))
    W = float(m["x_edges"][-1])
    counts = torch.as_tensor(m["counts"][:3])
    lmp = torch.full((3,), float(m["relative_to"]) * np.log(10.0), dtype=torch.float64)
    return counts, lmp, W


@pytest.mark.gpu
def test_committed_hit_maps():
    from geobipy_amd import hitmap
    counts, lmp, W = _fixture()
    h = counts.numpy()
    assert h.shape == (3, 250, 440) and int((h.sum(axis=1) == 0).sum()) == 39
    ref = mixtures.mixture_reference(h, W, max_components=4, n_iter=50)
    d = counts.cuda()
    got = hitmap.mixture(d, W, max_components=4, n_iter=50)
    _hold_stages_to(got, ref, 4, "committed maps")
    # the thresholds apart from the continuous comparison: the stopping rule on the device's own misfits, exactly
    f = mixtures.fit(d, lmp.cuda(), W, max_components=4, n_iter=50)
    want = _select_loop(got["misfit"].cpu().numpy())
    n = f["n_components"].cpu().numpy()
    assert n.dtype == np.int32 and np.array_equal(n, want)
    print("components selected (0 .. 4):", np.bincount(n.ravel(), minlength=5).tolist())
    assert int((n == 0).sum()) == 39
    # the selected components: those of the chosen stage, sorted, shifted by the prior mean
    shift = float(lmp[0]) / np.log(10.0)
    mean, weight = f["mean"].cpu().numpy(), f["weight"].cpu().numpy()
    gm, gw = got["mean"].cpu().numpy(), got["weight"].cpu().numpy()
    for b, z in [(0, 5), (1, 100), (2, 300), (0, 439)] + [tuple(i) for i in np.argwhere(n == n.max())[:3]]:
        k = n[b, z]
        s = k * (k - 1) // 2
        order = np.argsort(gm[b, s:s + k, z], kind="stable")
        assert np.allclose(mean[b, :k, z], gm[b, s:s + k, z][order] + shift, rtol=0.0, atol=1e-15) and np.isnan(mean[b, k:, z]).all()
        assert np.array_equal(weight[b, :k, z], gw[b, s:s + k, z][order])
    assert np.allclose(np.nansum(weight, axis=1)[n > 0], 1.0, rtol=0.0, atol=1e-12)


# -- end to end ----------------------------------------------------------------------------------------------------------------------

def _survey_arrays():
    from geobipy_amd import hdf, line_products as lp
    a, _ = hdf.load_results(SURVEY)
    hm = torch.as_tensor(a[lp.VALUES + "/values/data"])
    W = float(a[lp.VALUES + "/mesh/y/edges/data"][-1])
    de = np.asarray(a[lp.VALUES + "/mesh/z/edges/data"], dtype=np.float64)
    N = hm.shape[0]
    lmp = torch.as_tensor(np.broadcast_to(np.asarray(a[lp.VALUES + "/mesh/y/relative_to/data"], dtype=np.float64).reshape(-1), (N,)) * lp.LN10)
    return hm, lmp.contiguous(), W, de


def _same_fit(products, fit_, prefix):
    from geobipy_amd import line_products as lp
    for a, b in lp.MIXTURE_ENTRIES:
        want = fit_[b].cpu().numpy()
        got = products[prefix + a]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), prefix + a


@pytest.mark.gpu
def test_from_results_and_the_command_line_write_the_fits(tmp_path):
    import shutil
    from geobipy_amd import hitmap, intervals as iv, line_products as lp
    hm, lmp, W, de = _survey_arrays()
    N = hm.shape[0]
    plain = lp.from_results(SURVEY, block=3)
    got = lp.from_results(SURVEY, block=3, mixtures=dict(max_components=3))
    assert set(got) - set(plain) == {"mixture_" + a for a, _ in lp.MIXTURE_ENTRIES}
    for k in plain:                                                  # the other products are untouched
        assert np.asarray(plain[k]).tobytes() == np.asarray(got[k]).tobytes(), k
    want = mixtures.fit(hm.cuda(), lmp.cuda(), W, max_components=3)
    _same_fit(got, want, "mixture_")
    assert got["mixture_n"].shape == (N, de.size - 1) and got["mixture_n"].dtype == np.int32 and got["mixture_mean"].shape == (N, 3, de.size - 1)
    assert got["mixture_misfit"].shape == (N, 2, de.size - 1) and got["mixture_n"].max() >= 2
    # on an elevation axis the fits pass through: components have no identity across depth cells that a mean over cells could keep
    from geobipy_amd import hdf
    surface = np.asarray(hdf.load_results(SURVEY)[0]["/data/elevation/data"], dtype=np.float64).reshape(-1)
    on = lp.on_elevation(got, surface, edges=np.linspace(surface.min() - 60.0, surface.max(), 25))
    assert on["mean"].shape == (N, 24)
    for a, _ in lp.MIXTURE_ENTRIES:
        assert on["mixture_" + a] is got["mixture_" + a], a
    # with intervals: the fits of the units' marginals, through the int64 entry
    edges = [-2.0, 0.0, 10.0, 30.25, 75.0, 230.0]
    both = lp.from_results(SURVEY, intervals={"kind": "depth", "edges": edges}, mixtures=dict(max_components=4, n_iter=20))
    r = iv.depth_ranges(de, edges)
    marg = hitmap.interval_marginals(hm.cuda(), torch.as_tensor(r.lo), torch.as_tensor(r.hi))
    assert marg.dtype == torch.int64
    _same_fit(both, mixtures.fit(marg, lmp.cuda(), W, max_components=4, n_iter=20), "interval_mixture_")
    _same_fit(both, mixtures.fit(hm.cuda(), lmp.cuda(), W, max_components=4, n_iter=20), "mixture_")
    assert both["interval_mixture_mean"].shape == (N, 4, 5) and (both["interval_mixture_n"][:, 0] == 0).all() and r.n_cells[0] == 0
    assert np.isnan(both["interval_mixture_mean"][:, :, 0]).all() and (both["interval_mixture_n"][:, 1:] >= 1).all()
    # the command line
    first = str(tmp_path / "0.0.h5")
    shutil.copy(SURVEY, first)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.line_products", first, "--mixtures", "3"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    z = dict(np.load(lp.output_path(first)))
    assert set(z) == set(got)
    for k in got:
        assert np.asarray(z[k]).tobytes() == np.asarray(got[k]).tobytes(), k
    # global classes of the line feed the class probabilities
    g = mixtures.global_classes(dict(mixture_mean=z["mixture_mean"]), 3)
    mu, sd = lp.check_classes(g["means"], g["scales"])
    p = hitmap.class_probability(hm.cuda(), lmp.cuda(), W, mu, sd)["probability"].cpu().numpy()
    total = p.sum(axis=1)
    fin = np.isfinite(total)
    assert fin.any() and np.abs(total[fin] - 1.0).max() <= 1e-12
    with_classes = lp.from_results(SURVEY, classes=(mu, sd), mixtures=True)
    assert with_classes["class_probability"].shape == (N, 3, de.size - 1) and "mixture_n" in with_classes
