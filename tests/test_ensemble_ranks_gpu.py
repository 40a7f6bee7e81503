"""Ranks within columns on the device (csrc/gbp_ensemble_ranks.h k_series_ranks<PLAIN / RASTER, FOLD>; geobipy_amd.ensembles
series_ranks / ensemble_ranks / series_rank_diagnostics / rank_diagnostics / quantiles / correlation(rank=True)).

Every output of the kernel is an integer or a copy of an input double, so less, leq and order are held to the numpy rule
(ensembles.rank_counts_reference) with ``==``: the plain entry on its input, the raster entry on its own x_out (the values it ranked),
and x_out against np.log10 of the raster's rule within the 4 ulp the raster tests allow.  The diagnostics of the derived series go
through the existing kernel: they are held to the long-double rule on THE DEVICE'S z and indicator series copied to the host, within
the bounds tests/test_ensemble_diagnostics_gpu.py derives (ndtri's rounding is then nobody's tolerance), and the entries that
compose them must repeat those bits."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import ensembles
from geobipy_amd.ensembles import rank_counts_reference as rule
from test_ensemble_correlation_gpu import _check_sounding as _check_correlation
from test_ensemble_diagnostics_gpu import _check_sounding as _check_diagnostics
from test_ensemble_diagnostics_gpu import _hand_made, _numpy
from test_ensemble_ranks import columns
from test_rjmcmc_gpu import GOLDEN, _chains

U = 2.0 ** -52
P16 = tuple(np.linspace(0.0, 1.0, 16))


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _same(a, b):
    """== with NaN == NaN (order holds NaN where the rule has it)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _starts(segs, n_rows):
    M_max = max(1, max(m for m, _ in segs))
    start = np.zeros((len(segs), M_max), dtype=np.int32)
    for b, (m, n) in enumerate(segs):
        if m > 1 and b % 3 == 2:                                         # spread over the rows: unused rows between the segments
            start[b, :m] = np.linspace(0, n_rows - n, m).astype(np.int32)
            assert np.all(np.diff(start[b, :m]) >= n)
        else:
            start[b, :m] = ((n_rows - m * n) if b % 2 else 0) + n * np.arange(m)
    return start


def _args(x, start, segs):
    dev = _dev()
    return (torch.as_tensor(x).to(dev), torch.as_tensor(start).to(dev), torch.tensor([m for m, _ in segs], dtype=torch.int32, device=dev),
            torch.tensor([n for _, n in segs], dtype=torch.int32, device=dev))


def _check_counts(got, b, x, starts, n, fold, probs, label):
    want = rule(x, starts, n, fold=fold, probabilities=probs)
    for name in ("less", "leq"):
        assert _same(got[name][b], want[name]), (label, b, name, fold)
    if len(probs):
        assert _same(got["order"][b], want["order"]), (label, b, "order", fold)
    return want


# V, n_rows, (M, N) per sounding.  n = M N = 8, 14, 64, 66, 256, 258 and 2 060 used rows; the padded length P (32, 128, 512, 4 096) and with
# it the column tile T = 64, 64, 32, 4; V = 1, 63, 65, 257 and 9 across it (a partial tile, three, nine and three tiles); a sounding with
# M = 0 and one with N < 4; segments that start at row 0, end at the last row, or have unused rows between them.
CASES = [
    (1, 20, [(2, 4), (2, 7), (0, 0)]),
    (63, 70, [(2, 33), (1, 64), (2, 3)]),
    (65, 300, [(6, 43), (4, 64), (1, 300)]),
    (257, 260, [(2, 7), (6, 43), (2, 4)]),
    (9, 2100, [(2, 1030), (16, 131), (3, 700)]),
]


@pytest.mark.parametrize("V, n_rows, segs", CASES)
def test_plain_entry_is_the_rule(V, n_rows, segs):
    rng = np.random.default_rng(100 * V + n_rows)
    B = len(segs)
    x = rng.standard_normal((B, n_rows, V))
    start = _starts(segs, n_rows)
    for b in range(B):                                                   # the tie and extreme columns of the host tests
        w = min(V, 8)
        x[b, :, V - w:] = columns(rng, n_rows)[:, 8 - w:] if V < 8 else columns(rng, n_rows)
    if V > 8:
        x[0, start[0, 0] + 2, 0] = np.nan                                # a NaN in a used row: that column alone is refused
        x[1, start[1, 0] + 1, 1] = -np.inf
    free = np.setdiff1d(np.arange(n_rows), np.concatenate([np.arange(q, q + segs[2][1]) for q in start[2, :segs[2][0]]] + [np.zeros(0, dtype=int)]))
    if free.size and V > 8:
        x[2, free[0], 2] = np.nan                                        # a NaN in an unused row: nothing changes
    args = _args(x, start, segs)
    label = "plain V=%d rows=%d" % (V, n_rows)
    for fold in (False, True):
        for probs in ((), (0.5,), P16):
            got = _numpy(ensembles.series_ranks(*args, fold=fold, probabilities=probs, values=True))
            assert got["less"].dtype == np.int32 and got["less"].shape == (B, n_rows, V) and ("order" in got) == bool(len(probs))
            for b, (m, n) in enumerate(segs):
                want = _check_counts(got, b, x[b], start[b, :m], n, fold, probs, label)
                used = want["less"] >= 0
                live = m > 0 and n >= 4
                rows = np.zeros(n_rows, dtype=bool)
                for q in start[b, :m] if live else ():
                    rows[q:q + n] = True
                assert np.array_equal(got["x_out"][b][rows], x[b][rows], equal_nan=True) and np.isnan(got["x_out"][b][~rows]).all()
                assert np.all(got["leq"][b][used] > got["less"][b][used]) and np.all(got["leq"][b][used] <= m * n)
            again = _numpy(ensembles.series_ranks(*args, fold=fold, probabilities=probs, values=True))
            assert all(np.array_equal(_bits(got[name]), _bits(again[name])) for name in got)      # a second call: the same bits
    only = _numpy(ensembles.series_ranks(*args, probabilities=P16, counts=False))
    assert set(only) == {"order"} and _same(only["order"], got["order"])


def test_a_column_at_the_limit_of_16384_rows():
    rng = np.random.default_rng(16384)
    x = rng.standard_normal((1, 16384, 1))
    x[0, rng.integers(0, 16384, 3000), 0] = x[0, 5, 0]                   # a long run of ties
    for segs in ([(2, 8192)], [(16, 1000)]):
        start = _starts(segs, 16384)
        got = _numpy(ensembles.series_ranks(*_args(x, start, segs), fold=True, probabilities=(0.05, 0.5, 0.95)))
        _check_counts(got, 0, x[0], start[0], segs[0][1], True, (0.05, 0.5, 0.95), "limit")


def test_null_outputs_are_skipped_and_nothing_else_is_written():
    from geobipy_amd import _lib
    import ctypes
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(3)
    B, rows, V, Q, G = 2, 70, 65, 3, 256
    segs = [(2, 33), (3, 21)]
    x, start, m, n = _args(rng.standard_normal((B, rows, V)), _starts(segs, rows), segs)
    p = (ctypes.c_double * Q)(0.05, 0.5, 0.95)
    full = _numpy(ensembles.series_ranks(x, start, m, n, fold=True, probabilities=(0.05, 0.5, 0.95), values=True))
    sizes = dict(less=B * rows * V, leq=B * rows * V, order=B * Q * 2 * V, x_out=B * rows * V)
    for wanted in (("less", "leq"), ("order",), ("x_out",), ("less", "leq", "order", "x_out"), ()):
        buf = {name: (torch.full((sizes[name] + 2 * G,), -77, dtype=torch.int32, device=dev) if name in ("less", "leq")
                      else torch.full((sizes[name] + 2 * G,), -77.0, dtype=torch.float64, device=dev)) for name in sizes}
        ptr = lambda name: buf[name][G:].data_ptr() if name in wanted else None      # noqa: E731
        assert lib.gbp_series_ranks(B, rows, V, x.data_ptr(), 3, start.data_ptr(), m.data_ptr(), n.data_ptr(), 1, Q, p, ptr("less"), ptr("leq"),
                                    ptr("order"), ptr("x_out"), st) == 0, lib.gbp_last_error()
        torch.cuda.synchronize()
        for name in sizes:
            a = buf[name].cpu().numpy()
            assert np.all(a[:G] == -77) and np.all(a[-G:] == -77), (wanted, name)           # the guards around every buffer
            if name in wanted:
                assert np.array_equal(a[G:-G].reshape(full[name].shape), full[name], equal_nan=True), (wanted, name)
            else:
                assert np.all(a == -77), (wanted, name)


def _ensemble(k, edges, sigma, misfit, dev):
    return ensembles.Ensemble(*(torch.as_tensor(a).to(dev) for a in (k, edges, sigma, misfit)), (torch.as_tensor(k) > 0).sum(dim=1), 3,
                              torch.zeros(k.shape[0], dtype=torch.float64, device=dev))


@pytest.mark.parametrize("K, per, counts", [
    (30, 160, [[0], [7], [8], [131], [160]]),
    (64, 160, [[0], [7], [8], [131], [160]]),
    (30, 64, [[64, 0, 64], [64, 7, 33], [20, 21, 64], [3, 0, 7], [64, 64, 64]]),       # three chains: an unused one in the middle, ...
])
def test_raster_entry_is_the_rule_on_its_own_values(K, per, counts):
    """Hand-made ensembles (a half-space, k = K = 64, an interface exactly at a cell centre, chains filled to 0 / 7 / 8 / all slots,
    three chains with one unused): counts and order == the rule on x_out; x_out within 4 ulp of np.log10 of the raster's rule."""
    dev = _dev()
    C = len(counts[0])
    for n_depth in (1, 65, 440):
        rng = np.random.default_rng(1000 * K + 10 * C + n_depth)
        depth_edges = np.linspace(0.0, 110.0, n_depth + 1)
        k, edges, sigma, misfit = _hand_made(rng, K, per, counts, ensembles.centres(depth_edges))
        B = k.shape[0]
        ens = _ensemble(k, edges, sigma, misfit, dev)
        start, m, n, used = ensembles.segments(np.asarray(counts), per)
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = np.log10(ensembles.realisations_reference(k, edges, sigma, depth_edges))
        label = "raster K=%d C=%d n_depth=%d" % (K, C, n_depth)
        for fold, probs in ((False, (0.05, 0.5, 0.95)), (True, P16), (True, ())):
            got = _numpy(ensembles.ensemble_ranks(ens, depth_edges, chains=C, fold=fold, probabilities=probs, values=True))
            assert np.array_equal(got["n_chains_used"], used) and np.array_equal(got["segment_length"], n) and np.array_equal(got["n_segments"], m)
            for b in range(B):
                x = got["x_out"][b]
                rows = np.zeros(k.shape[1], dtype=bool)
                for q in start[b, :m[b]] if n[b] >= 4 else ():
                    rows[q:q + n[b]] = True
                assert np.isnan(x[~rows]).all() and np.isfinite(x[rows]).all(), (label, b)
                assert np.allclose(x[rows], ref[b][rows], rtol=4 * U, atol=0), (label, b)
                _check_counts(got, b, np.where(rows[:, None], x, 0.0), start[b, :m[b]], int(n[b]), fold, probs, label)
        for b in (0, 1) if C == 1 else (3,):                             # no usable chain
            assert np.all(got["less"][b] == -1) and np.isnan(got["x_out"][b]).all()
    # the half-space: every cell holds one series, so every cell holds one set of counts
    assert np.all(got["less"][2] == got["less"][2][:, :1]) and np.all(got["leq"][2] == got["leq"][2][:, :1])


def _segment_tensors(start, m, n, dev):
    return tuple(torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (start, m, n))


def _check_products(products, derived, seg, host_seg, max_lag, percentiles, label):
    """``products`` (a rank-diagnostics entry's answer, device) against the derived series ``derived`` = (less, leq, folded less,
    folded leq) on the device: each product repeats the bits of series_diagnostics on the series made here by the public expressions,
    and that answer is held to the long-double rule on the series copied to the host."""
    less, leq, fless, fleq = derived
    start, m, n = host_seg
    nu = ensembles._used_count(seg[1], seg[2], less)
    series = dict(bulk=ensembles.normal_scores(less, leq, nu), folded=ensembles.normal_scores(fless, fleq, nu))
    for q in percentiles:
        series[q] = ensembles.indicators(less, nu, q / 100.0)
    got = _numpy(products)
    for key, x in series.items():
        d = _numpy(ensembles.series_diagnostics(x, *seg, max_lag=max_lag))
        host = x.cpu().numpy()
        for b in range(host.shape[0]):
            xb = host[b].copy()
            rows = np.zeros(xb.shape[0], dtype=bool)
            for q in start[b, :m[b]]:
                rows[q:q + n[b]] = True
            xb[~rows] = 0.0                                              # (unused rows hold NaN: the rule does not read them)
            _check_diagnostics(d, b, xb, start[b, :m[b]], int(n[b]), max_lag, "%s %s" % (label, key))
        if key == "bulk":
            for name, src in (("rhat_bulk", "rhat"), ("ess_bulk", "ess"), ("tau_bulk", "tau"), ("truncated_bulk", "truncated")):
                assert np.array_equal(_bits(got[name]), _bits(d[src])), (label, name)
        elif key == "folded":
            assert np.array_equal(_bits(got["rhat_folded"]), _bits(d["rhat"])), label
        else:
            assert np.array_equal(_bits(got["ess_percentile_" + ensembles.percentile_name(key)]), _bits(d["ess"])), (label, key)
    assert np.array_equal(got["rhat_rank"], np.maximum(got["rhat_bulk"], got["rhat_folded"]), equal_nan=True)
    lo, hi = (got["ess_percentile_" + ensembles.percentile_name(q)] for q in (percentiles[0], percentiles[-1]))
    assert np.array_equal(got["ess_tail"], np.minimum(lo, hi), equal_nan=True)
    return got


def test_series_rank_diagnostics_against_the_long_double_rule():
    rng = np.random.default_rng(41)
    V, n_rows, segs = 70, 300, [(4, 64), (2, 150), (6, 43), (0, 0)]
    B = len(segs)
    x = rng.standard_normal((B, n_rows, V))
    for t in range(1, n_rows):                                           # AR(1), coefficient 0.8: no segment lies wholly on one side of a quantile
        x[:, t] = 0.8 * x[:, t - 1] + 0.6 * x[:, t]                      # (W = 0 and rhat = inf there, which the diagnostics' checker does not take)
    x[:, :, :8] = np.stack([columns(rng, n_rows) for _ in range(B)])
    x[0, :, 9] = np.round(x[0, :, 9])                                    # ties
    x[1, :, 10] = rng.standard_normal(n_rows) * np.where(np.arange(n_rows) < 150, 1.0, 3.0)      # two chains of one median, spreads 1 and 3
    start = _starts(segs, n_rows)
    args = _args(x, start, segs)
    qs = (5.0, 50.0, 95.0)
    plain = ensembles.series_ranks(*args, probabilities=[q / 100.0 for q in qs])
    folded = ensembles.series_ranks(*args, fold=True)
    products = ensembles.series_rank_diagnostics(*args, max_lag=63, percentiles=qs)
    host_seg = (start, np.array([m_ for m_, _ in segs]), np.array([n_ for _, n_ in segs]))
    got = _check_products(products, (plain["less"], plain["leq"], folded["less"], folded["leq"]), args[1:], host_seg, 63, qs, "series")
    assert got["rhat_folded"][1, 10] > got["rhat_bulk"][1, 10]
    assert np.isnan(got["ess_bulk"][3]).all() and np.isnan(got["quantile_50"][3]).all() and np.isnan(got["ess_bulk"][:, 4]).all()      # M = 0; all equal
    # the quantiles: the rule's order statistics, interpolated by the expression of the host reference
    for b, (m, n) in enumerate(segs[:3]):
        want = ensembles.rank_diagnostics_reference(x[b], start[b, :m], n, 63, percentiles=qs)
        for q in qs:
            name = "quantile_" + ensembles.percentile_name(q)
            assert np.array_equal(got[name][b], want[name], equal_nan=True), (b, name)
        c = np.concatenate([x[b, s_:s_ + n, 8:] for s_ in start[b, :m]])
        assert np.allclose(got["quantile_5"][b, 8:], np.quantile(c, 0.05, axis=0), rtol=2 * U, atol=2 * U * float(np.abs(c).max()))


def test_normal_scores_against_scipy():
    """One loose check of the device's ndtri: torch's CPU ndtri and scipy's differ by at most 8.9e-16 on the arguments (r - 3/8) / (n +
    1/4) of every midrank of n = 8 .. 16 384 (measured here, on the CPU, every time); the device may differ from scipy by four times
    that -- another implementation of the same function."""
    special = pytest.importorskip("scipy.special")
    dev = _dev()
    worst_cpu = worst_dev = 0.0
    for n in (8, 14, 64, 66, 256, 258, 2060, 16384):
        r = np.arange(1, 2 * n + 1) / 2.0                                # every midrank and half-rank
        less = torch.as_tensor(np.floor(r - 0.5).astype(np.int32))
        leq = torch.as_tensor((2 * r - 1).astype(np.int32)) - less       # (less + leq + 1) / 2 == r
        nu = torch.tensor(float(n), dtype=torch.float64)
        want = special.ndtri((r - 0.375) / (n + 0.25))
        cpu = ensembles.normal_scores(less, leq, nu).numpy()
        got = ensembles.normal_scores(less.to(dev), leq.to(dev), nu.to(dev)).cpu().numpy()
        worst_cpu = max(worst_cpu, float(np.max(np.abs(cpu - want))))
        worst_dev = max(worst_dev, float(np.max(np.abs(got - want))))
    print("ndtri: torch CPU - scipy %.3e, device - scipy %.3e" % (worst_cpu, worst_dev))
    assert worst_dev <= 4 * worst_cpu


def test_rank_diagnostics_quantiles_and_spearman_of_an_ensemble():
    dev = _dev()
    K, per, counts = 30, 64, [[64, 0, 64], [64, 7, 33], [20, 21, 64], [3, 0, 7], [64, 64, 64]]
    rng = np.random.default_rng(77)
    depth_edges = np.linspace(0.0, 110.0, 67)
    k, edges, sigma, misfit = _hand_made(rng, K, per, counts, ensembles.centres(depth_edges))
    ens = _ensemble(k, edges, sigma, misfit, dev)
    start, m, n, used = ensembles.segments(np.asarray(counts), per)
    seg = _segment_tensors(start, m, n, dev)
    qs = (5.0, 50.0, 95.0)
    plain = ensembles.ensemble_ranks(ens, depth_edges, chains=3, probabilities=[q / 100.0 for q in qs], values=True)
    folded = ensembles.ensemble_ranks(ens, depth_edges, chains=3, fold=True)
    products = ensembles.rank_diagnostics(ens, depth_edges, chains=3, max_lag=31, percentiles=qs)
    got = _check_products({name: v for name, v in products.items() if v.ndim == 2}, (plain["less"], plain["leq"], folded["less"], folded["leq"]),
                          seg, (start, m, n), 31, qs, "ensemble")
    all_ = _numpy(products)
    assert np.array_equal(all_["n_chains_used"], used) and np.array_equal(all_["segment_length"], n) and np.array_equal(all_["n_segments"], m)
    blocks = _numpy(ensembles.rank_diagnostics(ens, depth_edges, chains=3, max_lag=31, percentiles=qs, block=2))
    assert all(np.array_equal(_bits(blocks[name]), _bits(all_[name])) for name in all_)            # soundings in blocks: the same bits
    for b in range(5):
        fin = all_["ess_bulk"][b][np.isfinite(all_["ess_bulk"][b])]
        assert (np.isnan(all_["ess_bulk_min"][b]) and fin.size == 0) or all_["ess_bulk_min"][b] == fin.min()
    # the layer count and the misfit go through the plain entry
    two = torch.stack((ens.k.to(torch.float64), torch.log10(ens.misfit)), dim=2).contiguous()
    scalars = _numpy(ensembles.series_rank_diagnostics(two, *seg, max_lag=31, percentiles=qs))
    for name in scalars:
        assert np.array_equal(_bits(all_[name + "_k"]), _bits(scalars[name][:, 0])) and np.array_equal(_bits(all_[name + "_misfit"]), _bits(scalars[name][:, 1])), name
    # quantiles: the launch that writes no series gives the quantiles of rank_diagnostics, the rule's on x_out
    qd = _numpy(ensembles.quantiles(ens, depth_edges, qs, chains=3, block=2))
    x_out = plain["x_out"].cpu().numpy()
    for q in qs:
        name = "quantile_" + ensembles.percentile_name(q)
        assert np.array_equal(_bits(qd[name]), _bits(got[name])), name
    for b in (0, 1, 2, 4):
        want = ensembles.rank_diagnostics_reference(np.nan_to_num(x_out[b]), start[b, :m[b]], int(n[b]), 31, percentiles=qs)
        assert np.array_equal(got["quantile_95"][b], want["quantile_95"], equal_nan=True), b
    assert np.isnan(got["quantile_50"][3]).all()
    # Spearman: the correlation of the device's midranks, held to the long-double rule on them
    corr = _numpy(ensembles.correlation(ens, depth_edges, chains=3, band=20, rank=True))
    mid = ensembles.midranks(plain["less"], plain["leq"])
    same = _numpy(ensembles.series_correlation(mid, *seg, band=20))
    assert np.array_equal(_bits(corr["band"]), _bits(same["band"])) and np.array_equal(_bits(corr["sd"]), _bits(same["sd"]))
    host = np.nan_to_num(mid.cpu().numpy())
    for b in range(5):
        _check_correlation(corr, b, host[b], start[b, :m[b]], int(n[b]), 20, "spearman")
    ranked = _numpy(ensembles.series_correlation(plain["x_out"].nan_to_num(), *seg, band=20, rank=True))
    assert np.array_equal(_bits(ranked["band"]), _bits(corr["band"]))
    untouched = _numpy(ensembles.correlation(ens, depth_edges, chains=3, band=20))
    assert not np.array_equal(untouched["band"], corr["band"], equal_nan=True)


def _check_run(d, n_depth):
    """What every real run must show."""
    g = _numpy(d)
    nu = (g["n_segments"] * g["segment_length"]).astype(np.float64)[:, None]
    assert g["ess_bulk"].shape[1] == n_depth and np.all(g["n_segments"] >= 2) and np.all(g["segment_length"] >= 4)
    live = np.isfinite(g["ess_bulk"])
    assert live.any() and np.array_equal(live, np.isfinite(g["rhat_bulk"]))
    assert np.all(g["ess_bulk"][live] >= 1.0) and np.all((g["ess_bulk"] <= nu * np.log10(nu) * (1 + 8 * U))[live])
    assert np.all(g["rhat_bulk"][live] > 0.5)
    both = np.isfinite(g["rhat_bulk"]) & np.isfinite(g["rhat_folded"])
    assert np.all(g["rhat_rank"][both] == np.maximum(g["rhat_bulk"], g["rhat_folded"])[both])
    assert np.all(g["quantile_5"][live] <= g["quantile_50"][live]) and np.all(g["quantile_50"][live] <= g["quantile_95"][live])
    assert np.isfinite(g["ess_bulk_misfit"]).all() and np.isfinite(g["quantile_50_k"]).all()
    return g


def test_rank_diagnostics_of_real_chains_replicates_and_time_domain_chains():
    from geobipy_amd import replicates
    from geobipy_amd.tdem import TdemDeviceChains
    from test_tdem_sampler import OFFSET, _survey
    B, nk, thin = 16, 64, 2
    _, _, dc = _chains(B, 17, exact=True, hitmap=True, ensemble=dict(n_keep=nk, thin=thin))
    dc.run(60, accumulate=False)
    dc.run(nk * thin)
    edges = np.arange(dc.n_depth_bins + 1) * dc.depth_bin_width
    ens = ensembles.from_chains(dc)
    g = _check_run(ensembles.rank_diagnostics(ens, edges), dc.n_depth_bins)
    assert np.all(g["n_chains_used"] == 1) and np.all(g["n_segments"] == 2) and np.all(g["segment_length"] == nk // 2)
    r = _numpy(ensembles.ensemble_ranks(ens, edges, values=True))
    assert np.all(r["less"] >= 0) and np.all(r["less"] < r["leq"]) and np.all(r["leq"] <= nk)
    x = r["x_out"]
    want = rule(x[3], [0, nk // 2], nk // 2)
    assert _same(r["less"][3], want["less"]) and _same(r["leq"][3], want["leq"])
    ref = np.log10(ensembles.realisations_reference(ens.k.cpu().numpy(), ens.edges.cpu().numpy(), ens.sigma.cpu().numpy(), edges))
    assert np.allclose(x, ref, rtol=4 * U, atol=0)
    d = _numpy(ensembles.diagnostics(ens, edges))
    assert np.array_equal(np.isfinite(g["ess_bulk"]), np.isfinite(d["ess"]))                       # live cells are the diagnostics' live cells
    pooled = replicates.Pooled(dc, 2)
    p = _check_run(ensembles.rank_diagnostics(ensembles.from_chains(pooled), edges, chains=2, max_lag=15), dc.n_depth_bins)
    assert p["ess_bulk"].shape == (B // 2, dc.n_depth_bins) and np.all(p["n_chains_used"] == 2) and np.all(p["n_segments"] == 4)
    s, h, data, scale, opts, groups = _survey(4, seed=3)
    tc = TdemDeviceChains(s, h, data, OFFSET, seed=77, hitmap=True, ensemble=dict(n_keep=32, thin=4), **opts)
    tc.run(100, accumulate=False)
    tc.run(120)
    t = _check_run(ensembles.rank_diagnostics(ensembles.from_chains(tc), np.arange(tc.n_depth_bins + 1) * tc.depth_bin_width, max_lag=9), tc.n_depth_bins)
    assert np.all(t["segment_length"] == 15) and np.all(t["n_segments"] == 2)


def test_survey_and_command_lines_carry_the_rank_diagnostics(tmp_path):
    from geobipy_amd import survey
    from geobipy_amd.__main__ import main
    options = os.path.join(GOLDEN, "resolve_options_small")
    timings = {}
    res = survey.infer(options, exact_jacobian=True, ensemble=16, ensemble_rank_diagnostics=dict(max_lag=7), timings=timings)
    off = survey.infer(options, exact_jacobian=True, ensemble=16)
    S, nd = res["status"].size, res["mean_log10_conductivity"].shape[1]
    maps = ("ensemble_rhat_rank", "ensemble_ess_bulk", "ensemble_ess_tail")
    rows = tuple(n + s for n in maps for s in ("_k", "_misfit")) + ("ensemble_ess_bulk_min",)
    assert set(res) - set(off) == set(maps + rows) and set(off) - set(res) == set()          # keyword off: the keys of before
    for n in off:
        assert np.array_equal(np.asarray(res[n]), np.asarray(off[n]), equal_nan=True), n       # ... and the arrays of before
    assert all(res[n].shape == (S, nd) and res[n].dtype == np.float64 for n in maps) and all(res[n].shape == (S,) for n in rows) and "ensemble" in timings
    usable = (res["ensemble_k"] > 0).sum(axis=1) >= 8
    assert usable.any() and np.isnan(res["ensemble_ess_bulk"][~usable]).all() and np.isnan(res["ensemble_ess_bulk_min"][~usable]).all()
    assert np.isfinite(res["ensemble_ess_bulk_misfit"][usable]).all() and np.isfinite(res["ensemble_ess_bulk_min"][usable]).all()
    ess = res["ensemble_ess_bulk"][usable]
    assert np.all(ess[np.isfinite(ess)] >= 1.0)
    # the survey's command line, with replicates
    out = tmp_path / "cli"
    out.mkdir()
    assert main([options, str(out), "--exact-jacobian", "--no-containers", "--ensemble", "16", "--ensemble-rank-diagnostics", "7", "--replicates", "2"]) == 0
    ln = np.unique(res["line"])[0]
    line = np.load(str(out / "{}.npz".format(ln)))
    n_line = int((res["line"] == ln).sum())
    assert all(n in line.files and line[n].shape == (n_line, nd) for n in maps) and all(line[n].shape == (n_line,) for n in rows)
    # the module's command line on a saved ensemble
    _, _, dc = _chains(6, 5, exact=True, hitmap=True, ensemble=dict(n_keep=24, thin=2))
    dc.run(30, accumulate=False)
    dc.run(48)
    ens = ensembles.from_chains(dc)
    path = ensembles.save(ens, str(tmp_path / "run.npz"))
    axis = ["--depth-axis", str(dc.n_depth_bins), repr(float(dc.depth_bin_width))]
    edges = np.arange(dc.n_depth_bins + 1) * float(dc.depth_bin_width)
    written = ensembles.main([path] + axis + ["--rank", "--percentiles", "10", "90", "--max-lag", "5"])
    assert written == str(tmp_path / "run.rank_diagnostics.npz")
    f = np.load(written)
    want = _numpy(ensembles.rank_diagnostics(ens, edges, max_lag=5, percentiles=(10, 90)))
    assert all(np.array_equal(f[n], want[n], equal_nan=True) for n in want) and int(f["thin"]) == 2 and np.array_equal(f["percentiles"], [10.0, 90.0])
    assert "ess_percentile_10" in f.files and "quantile_90_misfit" in f.files
    written = ensembles.main([path] + axis + ["--correlation", "9", "--spearman"])
    f = np.load(written)
    want = _numpy(ensembles.correlation(ens, edges, band=9, rank=True))
    assert all(np.array_equal(f[n], want[n], equal_nan=True) for n in want)


def test_the_c_entries_refuse_bad_arguments_by_name():
    import ctypes
    from geobipy_amd import _lib
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    B, rows, V, K = 2, 20, 5, 6
    x = torch.zeros((B, rows, V), dtype=torch.float64, device=dev)
    start = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    m, n = torch.full((B,), 2, dtype=torch.int32, device=dev), torch.full((B,), 10, dtype=torch.int32, device=dev)
    less, leq = (torch.full((B, rows, V), 7, dtype=torch.int32, device=dev) for _ in range(2))
    order = torch.full((B, 16, 2, V), 7.0, dtype=torch.float64, device=dev)
    ptr = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    probs = lambda *v: (ctypes.c_double * max(len(v), 1))(*v)      # noqa: E731
    good = probs(0.05, 0.95)
    plain = lambda B_=B, rows_=rows, V_=V, x_=x, M=2, start_=start, m_=m, n_=n, nq=2, p_=good, less_=less, leq_=leq: lib.gbp_series_ranks(      # noqa: E731
        B_, rows_, V_, ptr(x_), M, ptr(start_), ptr(m_), ptr(n_), 0, nq, p_, ptr(less_), ptr(leq_), ptr(order), None, st)
    for kw in (dict(B_=-1), dict(rows_=0), dict(rows_=16385), dict(rows_=32769), dict(V_=0), dict(M=0), dict(M=17), dict(nq=-1), dict(nq=17),
               dict(p_=None), dict(p_=probs(0.5, 1.5)), dict(p_=probs(-0.1, 0.5)), dict(p_=probs(0.5, float("nan"))), dict(p_=probs(float("inf"), 0.5)),
               dict(x_=None), dict(start_=None), dict(m_=None), dict(n_=None), dict(less_=None), dict(leq_=None),
               dict(B_=4194304, V_=1)):                                                             # 2^22 workgroups of 1 024 threads
        assert plain(**kw) != 0 and b"gbp_series_ranks" in lib.gbp_last_error(), kw
    assert plain(B_=0, x_=None) == 0                                     # an empty block: OK without a launch
    k = torch.ones((B, rows), dtype=torch.int32, device=dev)
    e = torch.full((B, rows, K), float("inf"), dtype=torch.float64, device=dev)
    s = torch.ones((B, rows, K), dtype=torch.float64, device=dev)
    z = torch.linspace(0.5, 4.5, V, dtype=torch.float64, device=dev)
    raster = lambda B_=B, ns=rows, K_=K, k_=k, e_=e, s_=s, nd=V, z_=z, M=2, nq=2, p_=good, less_=less: lib.gbp_ensemble_ranks(      # noqa: E731
        B_, ns, K_, ptr(k_), ptr(e_), ptr(s_), nd, ptr(z_), M, ptr(start), ptr(m), ptr(n), 1, nq, p_, ptr(less_), ptr(leq), ptr(order), None, st)
    for kw in (dict(B_=-1), dict(ns=0), dict(ns=16385), dict(K_=0), dict(K_=65), dict(nd=0), dict(M=0), dict(M=17), dict(nq=-1), dict(nq=17),
               dict(p_=None), dict(p_=probs(0.5, 1.5)), dict(k_=None), dict(e_=None), dict(s_=None), dict(z_=None), dict(less_=None)):
        assert raster(**kw) != 0 and b"gbp_ensemble_ranks" in lib.gbp_last_error(), kw
    assert raster(B_=0, k_=None) == 0
    torch.cuda.synchronize()
    assert torch.all(less == 7) and torch.all(leq == 7) and torch.all(order == 7.0)              # nothing was written
    with pytest.raises(ValueError, match="overlap"):                     # the Python entry checks the lists it is given
        ensembles.series_ranks(x, start, m, torch.full((B,), 11, dtype=torch.int32, device=dev))
