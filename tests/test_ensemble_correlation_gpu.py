"""Correlation between depth cells on the device (csrc/gbp_ensemble_corr.h k_series_moments / k_series_correlation<PLAIN / RASTER> /
k_correlation_sd / k_correlation_finish / k_band_runs; geobipy_amd.ensembles series_correlation / correlation / correlation_runs;
DESIGN.md 3.22) against the rule ensembles.correlation_reference evaluated in long double -- never against device output.

Bounds (a priori: they hold for any order of summation; nothing here is a measurement of the kernel).  With U = 2^-52, n the used
rows of the sounding and r = max |x| / min sd over its live variables:
    eps = 8 (n + 8) U (1 + r)
    R     |d| <= eps                       C(u, v)   |d| <= eps sd_u sd_v
    sd    relative eps                     mean      |d| <= eps max |x|
(a centred product sum of n terms carries at most (n + 2) U of sum |d_u d_v| <= (n - 1) sd_u sd_v plus what the rounding of the mean,
(n + 1) U max |x| per centred value, does to it; the 8 covers both and the division and square roots of the normalisation.)  NaN
patterns exactly where the rule has them; the diagonal of a live variable == 1.0; a constant's sd == 0.0 and its mean the value as
stored.  Every case prints used / bound."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import ensembles
from geobipy_amd.ensembles import correlation_reference as rule
from geobipy_amd.ensembles import correlation_runs_reference as runs_rule
from test_ensemble_diagnostics_gpu import _hand_made, _series
from test_rjmcmc_gpu import GOLDEN, _chains

U = 2.0 ** -52
CH = 32                                                                  # rows per staged chunk (csrc/gbp_ensemble_corr.h CORR_CH)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: v.cpu().numpy() for n, v in d.items() if torch.is_tensor(v)}


def _check_sounding(got, b, x, starts, N, W, label, normalise=True, stored=True, min_sd=None):
    """Sounding b of the device's answer ``got`` (numpy: mean, sd, band) against the long-double rule on x [n_rows, V]; returns the
    number of live variables.  ``stored``: x holds the very doubles the device read (the raster entry takes its own log10)."""
    want = rule(x, starts, N, W, dtype=np.longdouble, normalise=normalise)
    w_band = want["band"].astype(np.float64)
    for n in ("mean", "sd"):
        assert np.array_equal(np.isnan(got[n][b]), np.isnan(want[n].astype(np.float64))), (label, b, n)
    assert np.array_equal(np.isnan(got["band"][b]), np.isnan(w_band)), (label, b, "band")
    sd = want["sd"].astype(np.float64)
    const = sd == 0.0
    live = sd > 0.0
    if const.any():
        assert np.all(got["sd"][b][const] == 0.0), (label, b)
        assert np.allclose(got["mean"][b][const], want["mean"][const].astype(np.float64), rtol=0 if stored else 4 * U, atol=0), (label, b)
    if not live.any():
        return 0
    n = len(starts) * N
    used = np.concatenate([x[q:q + N] for q in starts])[:, live]
    xmax = float(np.max(np.abs(used)))
    assert min_sd is None or float(sd[live].min()) >= min_sd, (label, b)
    r = xmax / float(sd[live].min())
    eps = 8 * (n + 8) * U * (1 + r)
    V = x.shape[1]
    scale = np.ones((V, W + 1))
    if not normalise:
        sdn = np.where(live, sd, np.nan)
        for j in range(W + 1):
            scale[:V - j, j] = sdn[:V - j] * sdn[j:]
    ok = ~np.isnan(w_band)
    d_band = float(np.max(np.abs(got["band"][b][ok].astype(np.longdouble) - want["band"][ok]) / scale[ok]))
    d_sd = float(np.max(np.abs(got["sd"][b][live].astype(np.longdouble) - want["sd"][live]) / want["sd"][live]))
    d_mean = float(np.max(np.abs(got["mean"][b][live].astype(np.longdouble) - want["mean"][live])))
    print("%s b=%d n=%d W=%d r=%.3g eps=%.2e used/bound: band %.3f sd %.3f mean %.3f" % (label, b, n, W, r, eps, d_band / eps, d_sd / eps, d_mean / (eps * xmax)))
    assert d_band <= eps, (label, b, "band", d_band, eps)
    assert d_sd <= eps, (label, b, "sd", d_sd, eps)
    assert d_mean <= eps * xmax, (label, b, "mean", d_mean, eps * xmax)
    if normalise:
        assert np.all(got["band"][b][live, 0] == 1.0), (label, b, "diagonal")
    return int(live.sum())


def _check_runs(band, threshold, depth_edges=None):
    """k_band_runs on the device band [B, V, W + 1] == the host rule; the resolution length >= the cell's thickness."""
    got = _numpy(ensembles.correlation_runs(band, threshold))
    host = band.cpu().numpy()
    for b in range(host.shape[0]):
        want = runs_rule(host[b], threshold)
        for n in want:
            assert got[n].dtype == want[n].dtype and np.array_equal(got[n][b], want[n]), (n, b)
    V = host.shape[1]
    edges = np.arange(V + 1) * 2.5 if depth_edges is None else depth_edges
    live = ~np.isnan(host[:, :, 0])
    length = ensembles.resolution_length(got["up"], got["down"], edges, live=live)
    assert np.array_equal(np.isnan(length), ~live) and np.all(length[live] >= np.broadcast_to(np.diff(edges), live.shape)[live])
    return got


# V, n_rows, (M, N) per sounding, W.  The boundaries of the implementation they cross: the 16-cell tile (15, 16, 17, 33); the strip of four
# tile rows (65: five tile rows, 70 and 130: a strip count that is not whole); the MFMA's 4 rows (n = 5, 6, 7, 9, 129); the chunk of CH
# = 32 staged rows (n = 31, 32, 33; 64 and 65); a tile diagonal partly inside the band (W = 1, 14, 17, 20); W = 0 and W = V - 1; the
# panel of eight tile diagonals (W = 129: ten diagonals, two panels, the strip's own columns staged beside the panel's).
CASES = [
    (1, 8, [(1, 8), (1, 4), (0, 0)], 0),
    (15, 9, [(2, 4), (1, 9), (1, 3)], 14),
    (16, 7, [(1, 7), (1, 5), (1, 6)], 15),
    (17, 40, [(2, 13), (3, 11), (1, 40)], 16),
    (33, 70, [(2, 35), (5, 14), (1, 69)], 1),
    (65, 130, [(2, 65), (4, 32), (1, 129)], 17),
    (130, 300, [(16, 18), (2, 150), (3, 100)], 64),
    (130, 300, [(16, 18), (2, 150), (3, 100)], 129),
    (70, 40, [(1, CH - 1), (1, CH), (1, CH + 1)], 20),
    (40, 70, [(2, CH), (1, 2 * CH + 1), (3, 21)], 39),
]


def _starts(segs, n_rows, gaps):
    M_max = max(1, max(m for m, _ in segs))
    start = np.zeros((len(segs), M_max), dtype=np.int32)
    for b, (m, n) in enumerate(segs):
        if gaps and m > 1:                                               # the segments spread over the rows: unused rows between them
            start[b, :m] = np.linspace(0, n_rows - n, m).astype(np.int32)
        else:
            start[b, :m] = ((n_rows - m * n) if b % 2 else 0) + n * np.arange(m)
    return start


def _args(x, start, segs):
    dev = _dev()
    return (torch.as_tensor(x).to(dev), torch.as_tensor(start).to(dev), torch.tensor([m for m, _ in segs], dtype=torch.int32, device=dev),
            torch.tensor([n for _, n in segs], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("V, n_rows, segs, W", CASES)
def test_plain_entry_against_the_rule(V, n_rows, segs, W):
    rng = np.random.default_rng(100 * V + n_rows + W)
    B = len(segs)
    x = _series(rng, B, n_rows, V)
    start = _starts(segs, n_rows, gaps=V == 17)
    if V == 17:
        assert start[0, 1] > start[0, 0] + segs[0][1] and start[1, 1] > start[1, 0] + segs[1][1]
    if V >= 3:
        x[0, :, 1] = 0.1 + 0.2                                           # a constant variable
        x[0, start[0, 0] + 2, 2] = np.nan                                # a NaN in a used row
    else:
        x[1, :, 0] = -2.5
    args = _args(x, start, segs)
    got = _numpy(ensembles.series_correlation(*args, band=W))
    assert got["band"].shape == (B, V, W + 1) and got["mean"].shape == (B, V) and got["sd"].shape == (B, V)
    label = "plain V=%d rows=%d" % (V, n_rows)
    for b, (m, n) in enumerate(segs):
        _check_sounding(got, b, x[b], start[b, :m], n, W, label, min_sd=0.05)
    cov = _numpy(ensembles.series_correlation(*args, band=W, normalise=False))
    for b, (m, n) in enumerate(segs):
        _check_sounding(cov, b, x[b], start[b, :m], n, W, label + " cov", normalise=False)
    assert np.array_equal(cov["sd"], got["sd"], equal_nan=True) and np.array_equal(cov["mean"], got["mean"], equal_nan=True)
    again = _numpy(ensembles.series_correlation(*args, band=W))
    for n in got:                                                        # a second call: the same bits
        assert np.array_equal(got[n].view(np.int64), again[n].view(np.int64)), n
    if V >= 3:
        full = _numpy(ensembles.series_correlation(*args))               # band=None: V - 1; the narrower band is its first columns
        assert full["band"].shape == (B, V, V) and np.array_equal(full["band"][:, :, :W + 1], got["band"], equal_nan=True)
    # a NaN in a row no segment uses changes nothing
    m0, n0 = segs[0]
    unused = np.ones(n_rows, dtype=bool)
    for q in start[0, :m0]:
        unused[q:q + n0] = False
    if unused.any():
        y = x.copy()
        y[0, np.nonzero(unused)[0][0], :] = np.nan
        other = _numpy(ensembles.series_correlation(torch.as_tensor(y).to(_dev()), *args[1:], band=W))
        assert all(np.array_equal(other[n].view(np.int64), got[n].view(np.int64)) for n in got)
    # the runs of the device's own band
    band = torch.as_tensor(got["band"]).to(_dev())
    for threshold in (0.5, -0.25):
        _check_runs(band, threshold)


def test_a_large_offset_and_exactly_linear_columns():
    """x = 1e6 + 0.05 noise: r = 2e7, and an uncentred sum xy - n mu mu would lose 1e12 / 0.0025 = 4e14 of its 4.5e15: the bound, eps =
    8 (n + 8) U 2e7 ~ 3e-6 here, fails it by orders of magnitude.  Columns that are exact affine images of another give +-1."""
    rng = np.random.default_rng(7)
    B, n_rows, V = 2, 80, 37
    x = 1e6 + 0.05 * rng.standard_normal((B, n_rows, V))
    x[1] = _series(rng, 1, n_rows, V)[0]
    x[1, :, 5] = -2.0 * x[1, :, 3] + 0.5                                 # exact in binary: a power of two and a short constant
    x[1, :, 9] = 4.0 * x[1, :, 3] - 1.0
    segs = [(2, 40), (3, 26)]
    start = _starts(segs, n_rows, gaps=False)
    got = _numpy(ensembles.series_correlation(*_args(x, start, segs), band=12))
    for b, (m, n) in enumerate(segs):
        _check_sounding(got, b, x[b], start[b, :m], n, 12, "offset" if b == 0 else "linear", min_sd=0.04)
    eps = 8 * (78 + 8) * U * (1 + 8.0 / 0.05)
    assert abs(got["band"][1, 3, 2] + 1.0) <= eps and abs(got["band"][1, 3, 6] - 1.0) <= eps and abs(got["band"][1, 5, 4] + 1.0) <= eps


def test_the_runs_kernel_on_hand_made_bands():
    dev = _dev()
    V = 9
    bands = []
    for W in (0, 3, V - 1):
        b = np.full((4, V, W + 1), 1.0)
        rng = np.random.default_rng(W)
        b[1] = rng.uniform(-1.0, 1.0, b[1].shape)
        b[1, :, 0] = 1.0
        b[2] = 0.75                                                      # the threshold hit exactly
        b[3, 4] = np.nan                                                 # a dead cell: its row and every entry that involves it
        for j in range(1, W + 1):
            if 4 - j >= 0:
                b[3, 4 - j, j] = np.nan
        for c in range(V):
            b[:, c, V - c:] = np.nan
        bands.append(b)
        got = _check_runs(torch.as_tensor(b).to(dev), 0.75, depth_edges=np.cumsum(np.r_[0.0, rng.uniform(0.5, 3.0, V)]))
        assert not got["closed_up"][0].any() and not got["closed_down"][0].any() and np.array_equal(got["down"][0], np.minimum(W, V - 1 - np.arange(V)))
        assert np.array_equal(got["down"][2], got["down"][0]) and np.array_equal(got["up"][2], got["up"][0])
        assert got["up"][3, 4] == 0 and got["down"][3, 4] == 0 and not got["closed_up"][3, 4] and not got["closed_down"][3, 4]
        if W:
            assert got["closed_down"][3, 3] and got["down"][3, 3] == 0 and got["closed_up"][3, 5] and got["up"][3, 5] == 0
    empty = ensembles.correlation_runs(torch.zeros((0, 5, 3), dtype=torch.float64, device=dev), 0.5)
    assert empty["up"].shape == (0, 5) and empty["closed_up"].dtype == torch.bool


def _ensemble(k, edges, sigma, misfit, dev):
    B = k.shape[0]
    return ensembles.Ensemble(*(torch.as_tensor(a).to(dev) for a in (k, edges, sigma, misfit)), (torch.as_tensor(k) > 0).sum(dim=1), 3,
                              torch.zeros(B, dtype=torch.float64, device=dev))


@pytest.mark.parametrize("K, per, counts", [
    (30, 160, [[0], [7], [8], [131], [160]]),
    (64, 160, [[0], [7], [8], [131], [160]]),
    (30, 64, [[64, 0, 64], [64, 7, 33], [20, 21, 64], [3, 0, 7], [64, 64, 64]]),       # three chains: an unused one in the middle, ...
])
def test_raster_entry_against_the_rule(K, per, counts):
    """_hand_made's soundings: 2 a half-space whose conductivity moves (every cell the same series: R = 1 throughout), 3 an interface
    exactly at a cell centre, 4 k = K in every slot and a deepest layer that never changes; counts 0 / 7 (no usable chain) / 8 / full."""
    dev = _dev()
    C = len(counts[0])
    for n_depth, W in ((1, 0), (65, 64), (130, 129), (440, 20)):        # 130, 129: two panels, and panel 0 stages 144 columns (three lane groups)
        rng = np.random.default_rng(1000 * K + 10 * C + n_depth)
        depth_edges = np.linspace(0.0, 110.0, n_depth + 1)
        z = ensembles.centres(depth_edges)
        k, edges, sigma, misfit = _hand_made(rng, K, per, counts, z)
        B = k.shape[0]
        ens = _ensemble(k, edges, sigma, misfit, dev)
        out = ensembles.correlation(ens, depth_edges, chains=C, band=W + 7 if n_depth == 65 else W, threshold=0.6, block=2 if n_depth == 65 else None)
        got = _numpy(out)
        start, m, n, used = ensembles.segments(np.asarray(counts), per)
        assert np.array_equal(got["n_chains_used"], used) and np.array_equal(got["segment_length"], n) and np.array_equal(got["n_segments"], m)
        assert got["band"].shape == (B, n_depth, W + 1) and got["resolution_length"].shape == (B, n_depth) and got["up"].dtype == np.int32
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.log10(ensembles.realisations_reference(k, edges, sigma, depth_edges))         # [B, slots, n_depth]
        label = "raster K=%d C=%d n_depth=%d" % (K, C, n_depth)
        for b in range(B):
            _check_sounding(got, b, x[b], start[b, :m[b]], int(n[b]), W, label, stored=False)
        # the same series written out and sent through the plain entry: two evaluations, each within eps of the rule
        seg = tuple(torch.as_tensor(a).to(dev) for a in (start, m, n))
        plain = _numpy(ensembles.series_correlation(ensembles.realisations(ens, depth_edges), *seg, band=W))
        assert np.array_equal(np.isnan(plain["band"]), np.isnan(got["band"]))
        for b in range(B):
            if m[b] == 0:
                continue
            _check_sounding(plain, b, x[b], start[b, :m[b]], int(n[b]), W, label + " plain", stored=False)
        # soundings without a usable chain: nothing; the half-space: constant; deep cells under every interface: constant
        for b in (0, 1) if C == 1 else (3,):
            assert all(np.isnan(got[name][b]).all() for name in ("mean", "sd", "band", "resolution_length"))
            assert not got["up"][b].any() and not got["down"][b].any() and not got["resolution_closed"][b].any()
        assert np.all(got["sd"][2] > 0.0) and np.nanmin(got["band"][2]) >= 1.0 - 1e-9 and not got["resolution_closed"][2].any()
        assert np.all(got["resolution_cells"][2] == np.minimum(W, np.arange(n_depth)) + np.minimum(W, n_depth - 1 - np.arange(n_depth)) + 1)
        deep = z > 60.0
        if deep.any():
            assert np.all(got["sd"][4][deep] == 0.0) and np.allclose(got["mean"][4][deep], np.log10(0.0125), rtol=4 * U, atol=0)
            assert np.isnan(got["band"][4][deep]).all()
        # the runs, the lengths and the flags follow from the band by the host rule
        for b in range(B):
            want = runs_rule(got["band"][b], 0.6)
            assert all(np.array_equal(got[name][b], want[name]) for name in want), (label, b)
        live = ~np.isnan(got["band"][:, :, 0])
        assert np.array_equal(got["resolution_cells"], got["up"] + got["down"] + 1)
        assert np.array_equal(got["resolution_closed"], got["closed_up"] & got["closed_down"])
        assert np.array_equal(got["resolution_length"], ensembles.resolution_length(got["up"], got["down"], depth_edges, live=live), equal_nan=True)
        assert np.all(got["resolution_length"][live] >= 110.0 / n_depth * (1 - 1e-12))
        dropped = _numpy(ensembles.correlation(ens, depth_edges, chains=C, band=W, threshold=0.6, keep_band=False, block=3))
        assert "band" not in dropped and all(np.array_equal(dropped[name], got[name], equal_nan=True) for name in dropped)


def test_a_two_layer_model_in_closed_form():
    """One interface that takes 8 distinct depths over 8 slots: the cells it sweeps are nested indicators, cell c is in the upper layer
    in a share p_c of the slots (p falls with depth), so R(a, b) = sqrt(p_b (1 - p_a) / (p_a (1 - p_b))) for a above b.  Beside it a
    half-space that never changes: every cell constant, sd 0, the band NaN."""
    dev = _dev()
    K, ns, nd = 2, 8, 10
    order = np.array([3, 0, 6, 1, 7, 4, 2, 5])
    k = np.array([[2] * ns, [1] * ns], dtype=np.int32)
    edges, sigma = np.full((2, ns, K), np.inf), np.full((2, ns, K), np.nan)
    edges[0, :, 0] = 1.0 + order                                         # 1 .. 8 m; the centres are 0.5 .. 9.5 m
    sigma[0, :, 0], sigma[0, :, 1] = 0.1, 0.01
    sigma[1, :, 0] = 0.05
    depth_edges = np.arange(nd + 1.0)
    got = _numpy(ensembles.correlation(_ensemble(k, edges, sigma, np.ones((2, ns)), dev), depth_edges, band=nd - 1))
    assert np.all(got["sd"][1] == 0.0) and np.isnan(got["band"][1]).all() and np.isnan(got["resolution_length"][1]).all()
    assert np.allclose(got["mean"][1], np.log10(0.05), rtol=4 * U, atol=0) and not got["up"][1].any() and not got["resolution_closed"][1].any()
    assert got["segment_length"][0] == 4 and got["n_segments"][0] == 2
    p = np.array([(edges[0, :, 0] > zc).mean() for zc in ensembles.centres(depth_edges)])
    live = (p > 0) & (p < 1)
    assert np.array_equal(live, [False] + [True] * 7 + [False] * 2) and np.array_equal(got["sd"][0] > 0, live)
    sd_min = np.sqrt(8.0 / 7.0 * (1.0 / 8.0) * (7.0 / 8.0))
    eps = 8 * (8 + 8) * U * (1 + 2.0 / sd_min)
    worst = 0.0
    for a in range(nd):
        for j in range(nd - a):
            b = a + j
            if live[a] and live[b]:
                want = 1.0 if j == 0 else np.sqrt(p[b] * (1 - p[a]) / (p[a] * (1 - p[b])))
                worst = max(worst, abs(got["band"][0, a, j] - want))
            else:
                assert np.isnan(got["band"][0, a, j])
    print("two layers: used/bound %.3f" % (worst / eps))
    assert worst <= eps
    assert np.allclose(got["sd"][0][live], np.sqrt(8.0 / 7.0 * p[live] * (1 - p[live])), rtol=eps, atol=0)


def _against_diagnostics(ens, edges, chains, label):
    """The correlation's mean and the diagnostics' mean are both within the bound's mean term of the pooled mean."""
    c, d = _numpy(ensembles.correlation(ens, edges, chains=chains, band=8)), _numpy(ensembles.diagnostics(ens, edges, chains=chains, max_lag=7))
    assert np.array_equal(c["segment_length"], d["segment_length"]) and np.array_equal(c["n_segments"], d["n_segments"])
    live = c["sd"] > 0
    assert live.any() and np.array_equal(np.isnan(c["mean"]), np.isnan(d["mean"])) and np.array_equal(live, d["sd"] > 0)
    n = (c["segment_length"] * c["n_segments"]).astype(np.float64)[:, None]
    xmax = np.nanmax(np.abs(c["mean"])) + 8 * np.nanmax(c["sd"])          # (a sample lies within sqrt(n) sd of the mean; sqrt(n) <= 8 here)
    eps = 8 * (n + 8) * U * (1 + xmax / c["sd"][live].min())
    assert np.all((np.abs(c["mean"] - d["mean"]) <= 2 * eps * xmax)[live]), label
    assert np.array_equal(c["mean"][c["sd"] == 0], d["mean"][c["sd"] == 0])
    assert np.all(c["band"][live][:, 0] == 1.0) and np.nanmax(np.abs(c["band"])) <= 1.0 + 1e-12
    assert np.all(c["resolution_length"][live] >= float(edges[1] - edges[0]) * (1 - 1e-12)) and np.all(c["resolution_cells"][live] >= 1)
    return c


def test_correlation_of_real_chains_and_of_replicates():
    from geobipy_amd import replicates
    B, nk, thin = 16, 32, 2
    _, _, dc = _chains(B, 17, exact=True, hitmap=True, ensemble=dict(n_keep=nk, thin=thin))
    dc.run(60, accumulate=False)
    dc.run(nk * thin)
    edges = np.arange(dc.n_depth_bins + 1) * dc.depth_bin_width
    ens = ensembles.from_chains(dc)
    assert torch.all(ens.count == nk)
    c = _against_diagnostics(ens, edges, 1, "real chains")
    assert c["band"].shape == (B, dc.n_depth_bins, 9) and np.all(c["n_chains_used"] == 1)
    x = np.log10(ensembles.realisations_reference(ens.k.cpu().numpy(), ens.edges.cpu().numpy(), ens.sigma.cpu().numpy(), edges))
    _check_sounding(c, 3, x[3], [0, nk // 2], nk // 2, 8, "real chains", stored=False)
    p = _against_diagnostics(ensembles.from_chains(replicates.Pooled(dc, 2)), edges, 2, "replicates")
    assert p["band"].shape == (B // 2, dc.n_depth_bins, 9) and np.all(p["n_chains_used"] == 2) and np.all(p["n_segments"] == 4)
    xs = x.reshape(B // 2, 2 * nk, -1)
    _check_sounding(p, 1, xs[1], [0, nk // 2, nk, nk + nk // 2], nk // 2, 8, "replicates", stored=False)


def test_correlation_of_time_domain_chains():
    from geobipy_amd.tdem import TdemDeviceChains
    from test_tdem_sampler import OFFSET, _survey
    B = 4
    s, h, data, scale, opts, groups = _survey(B, seed=3)
    dc = TdemDeviceChains(s, h, data, OFFSET, seed=77, hitmap=True, ensemble=dict(n_keep=32, thin=4), **opts)
    dc.run(100, accumulate=False)
    dc.run(120)
    edges = np.arange(dc.n_depth_bins + 1) * dc.depth_bin_width
    c = _against_diagnostics(ensembles.from_chains(dc), edges, 1, "time domain")
    assert np.all(c["segment_length"] == 15) and np.all(c["n_segments"] == 2)


def test_survey_and_command_lines_carry_the_correlation(tmp_path):
    from geobipy_amd import survey
    from geobipy_amd.__main__ import main
    options = os.path.join(GOLDEN, "resolve_options_small")
    timings = {}
    res = survey.infer(options, exact_jacobian=True, ensemble=16, ensemble_correlation=dict(band=12, keep_band=True), timings=timings)
    off = survey.infer(options, exact_jacobian=True, ensemble=16)
    S, nd = res["status"].size, res["mean_log10_conductivity"].shape[1]
    maps = ("ensemble_resolution_length", "ensemble_resolution_cells", "ensemble_resolution_closed")
    assert set(res) - set(off) == set(maps + ("ensemble_correlation_band",)) and set(off) - set(res) == set()
    for n in off:
        assert np.array_equal(np.asarray(res[n]), np.asarray(off[n]), equal_nan=True), n       # keyword off: the arrays of before
    assert all(res[n].shape == (S, nd) for n in maps) and res["ensemble_correlation_band"].shape == (S, nd, 13) and "ensemble" in timings
    assert res["ensemble_resolution_length"].dtype == np.float64 and res["ensemble_resolution_cells"].dtype == np.int32
    assert res["ensemble_resolution_closed"].dtype == bool
    usable = (res["ensemble_k"] > 0).sum(axis=1) >= 8
    live = ~np.isnan(res["ensemble_correlation_band"][:, :, 0])
    width = float(res["depth_bin_width"])
    assert usable.any() and not live[~usable].any() and live[usable].any()
    assert np.array_equal(np.isnan(res["ensemble_resolution_length"]), ~live)
    assert np.allclose(res["ensemble_resolution_length"][live], res["ensemble_resolution_cells"][live] * width, rtol=1e-12, atol=0)
    for s in np.nonzero(usable)[0][:3]:
        want = runs_rule(res["ensemble_correlation_band"][s], 0.5)
        assert np.array_equal(res["ensemble_resolution_cells"][s], want["up"] + want["down"] + 1)
        assert np.array_equal(res["ensemble_resolution_closed"][s], want["closed_up"] & want["closed_down"])
    # the survey's command line, with replicates
    out = tmp_path / "cli"
    out.mkdir()
    assert main([options, str(out), "--exact-jacobian", "--no-containers", "--ensemble", "16", "--ensemble-correlation", "7", "0.4", "--replicates", "2"]) == 0
    ln = np.unique(res["line"])[0]
    line = np.load(str(out / "{}.npz".format(ln)))
    n_line = int((res["line"] == ln).sum())
    assert all(n in line.files and line[n].shape == (n_line, nd) for n in maps) and "ensemble_correlation_band" not in line.files
    # the module's command line on a saved ensemble
    _, _, dc = _chains(6, 5, exact=True, hitmap=True, ensemble=dict(n_keep=24, thin=2))
    dc.run(30, accumulate=False)
    dc.run(48)
    ens = ensembles.from_chains(dc)
    path = ensembles.save(ens, str(tmp_path / "run.npz"))
    written = ensembles.main([path, "--depth-axis", str(dc.n_depth_bins), repr(float(dc.depth_bin_width)), "--correlation", "11", "--threshold", "0.7"])
    assert written == str(tmp_path / "run.correlation.npz") and not os.path.exists(str(tmp_path / "run.diagnostics.npz"))
    f = np.load(written)
    want = _numpy(ensembles.correlation(ens, np.arange(dc.n_depth_bins + 1) * float(dc.depth_bin_width), band=11, threshold=0.7))
    assert all(np.array_equal(f[n], want[n], equal_nan=True) for n in want) and int(f["thin"]) == 2 and float(f["threshold"]) == 0.7


def test_the_c_entries_refuse_bad_arguments_by_name():
    from geobipy_amd import _lib
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    B, rows, V, K, W = 2, 20, 5, 6, 3
    x = torch.zeros((B, rows, V), dtype=torch.float64, device=dev)
    start = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    m, n = torch.full((B,), 2, dtype=torch.int32, device=dev), torch.full((B,), 10, dtype=torch.int32, device=dev)
    stats = torch.full((B, 2, V), 7.0, dtype=torch.float64, device=dev)
    band = torch.full((B, V, W + 1), 7.0, dtype=torch.float64, device=dev)
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    plain = lambda B_=B, rows_=rows, V_=V, x_=x, M=2, start_=start, m_=m, n_=n, W_=W, stats_=stats, band_=band: lib.gbp_series_correlation(      # noqa: E731
        B_, rows_, V_, p(x_), M, p(start_), p(m_), p(n_), W_, 1, p(stats_), p(band_), st)
    for kw in (dict(B_=-1), dict(rows_=0), dict(rows_=32769), dict(V_=0), dict(M=0), dict(M=17), dict(W_=-1), dict(W_=V), dict(x_=None),
               dict(start_=None), dict(m_=None), dict(n_=None), dict(stats_=None), dict(band_=None)):
        assert plain(**kw) != 0 and b"gbp_series_correlation" in lib.gbp_last_error(), kw
    assert plain(B_=0, x_=None) == 0                                     # an empty block: OK without a launch
    k = torch.ones((B, rows), dtype=torch.int32, device=dev)
    e = torch.full((B, rows, K), float("inf"), dtype=torch.float64, device=dev)
    s = torch.ones((B, rows, K), dtype=torch.float64, device=dev)
    z = torch.linspace(0.5, 4.5, V, dtype=torch.float64, device=dev)
    raster = lambda B_=B, ns=rows, K_=K, k_=k, e_=e, s_=s, nd=V, z_=z, M=2, W_=W, stats_=stats, band_=band: lib.gbp_ensemble_correlation(      # noqa: E731
        B_, ns, K_, p(k_), p(e_), p(s_), nd, p(z_), M, p(start), p(m), p(n), W_, 1, p(stats_), p(band_), st)
    for kw in (dict(B_=-1), dict(ns=0), dict(ns=32769), dict(K_=0), dict(K_=65), dict(nd=0), dict(M=0), dict(M=17), dict(W_=-1), dict(W_=V),
               dict(k_=None), dict(e_=None), dict(s_=None), dict(z_=None), dict(stats_=None), dict(band_=None)):
        assert raster(**kw) != 0 and b"gbp_ensemble_correlation" in lib.gbp_last_error(), kw
    assert raster(B_=0, k_=None) == 0
    up, down = torch.full((B, V), 7, dtype=torch.int32, device=dev), torch.full((B, V), 7, dtype=torch.int32, device=dev)
    closed = torch.full((B, 2, V), 7, dtype=torch.uint8, device=dev)
    runs = lambda B_=B, V_=V, W_=W, band_=band, t=0.5, up_=up, down_=down, closed_=closed: lib.gbp_band_runs(      # noqa: E731
        B_, V_, W_, p(band_), t, p(up_), p(down_), p(closed_), st)
    for kw in (dict(B_=-1), dict(V_=0), dict(W_=-1), dict(W_=V), dict(t=float("nan")), dict(band_=None), dict(up_=None), dict(down_=None),
               dict(closed_=None)):
        assert runs(**kw) != 0 and b"gbp_band_runs" in lib.gbp_last_error(), kw
    assert runs(B_=0, band_=None) == 0
    torch.cuda.synchronize()
    assert torch.all(stats == 7.0) and torch.all(band == 7.0) and torch.all(up == 7) and torch.all(down == 7) and torch.all(closed == 7)       # nothing was written
    bad = start.clone()
    bad[1, 1] = 11                                                       # 11 + 10 > 20 rows: the Python entry checks the lists it is given
    with pytest.raises(ValueError, match="segment"):
        ensembles.series_correlation(x, bad, m, n)
