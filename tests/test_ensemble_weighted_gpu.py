"""Weighted per-column products on the device (csrc/gbp_ensemble_weighted.h k_series_weighted<plain / raster>; geobipy_amd.ensembles
series_weighted / weighted; geobipy_amd.sections lateral_products).

The weights are integers, so ``total``, ``quantile`` and ``above`` are held to ``ensembles.weighted_reference`` with ``==`` and the NaN
patterns must be equal: the plain entry on its input, the raster entry on the values the device itself rasters (gbp_ensemble_ranks'
x_out: the same expression of the same doubles).

``mean`` and ``sd`` are sums in fp64 whose order is not part of the rule; they are held to the rule in long double within a bound
stated here a priori, from the inputs and the rule alone.  With m = n_used, W = sum q, U = 2^-52:
    mean   |dev - ref| <= delta = (m + 2) U sum q |x| / W
           (m products, m - 1 additions, one division: at most (m + 1) roundings of 2^-53 each on a sum of magnitude sum q |x|)
    sd^2   |dev^2 - var| <= (m + 4) U sum q d^2 / W + 2 delta sum q |d| / W + delta^2,   d = x - mean_ref
           (a subtraction, a square, a product, m - 1 additions, a division, a square root squared again: (m + 5) roundings of 2^-53;
           a mean off by delta moves sum q (d - delta)^2 / W by at most 2 delta sum q |d| / W + delta^2)
Every case prints used / bound."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, ensembles, sections
from test_ensemble_weighted import DEPTH_EDGES_LINE, ONE, check_planted_products
from test_families_gpu import _dev, _to_device
from test_rjmcmc_gpu import GOLDEN
from test_sections import Z1_LINE, planted_line

U = 2.0 ** -52
PERCENTILES = (0, 5, 50, 95, 100)
PROBABILITIES = [q / 100.0 for q in PERCENTILES]
LEVELS = np.array([-3.0, -2.0, -1.0, 0.0, 1.0])                        # five levels: ties abound
SIZES, WIDTHS = [1, 2, 63, 64, 65, 257, 1024, 4096], [1, 3, 64, 65]
B = 3


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _listed(rng, n, n_rows, V):
    """rows int32 [B, n] in scrambled order with -1 past n_used, n_used ragged (0 and 1 among them), q int64 [B, n]: a third 0, one at
    2^40, small and large multiplicities among the rest; a row of weight 0 may name anything."""
    n_used = np.array([n, 1, 0] if V in (1, 64) else [max(n - n // 3, 1), 0, n], dtype=np.int32)
    rows = np.full((B, n), -1, dtype=np.int32)
    q = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        m = int(n_used[b])
        rows[b, :m] = rng.permutation(n_rows)[:m]
        w = np.where(rng.uniform(size=m) < 0.5, rng.integers(1, 6, m), rng.integers(1, ONE, m))
        w[rng.uniform(size=m) < 1.0 / 3.0] = 0
        if m:
            w[rng.integers(m)] = ONE
        q[b, :m] = w
        zero = np.nonzero(w == 0)[0]
        if zero.size:
            rows[b, zero[0]] = n_rows + 5                                # q == 0: outside the rows, never loaded
        q[b, m:] = 7                                                   # past n_used: no part
    return rows, n_used, q


def _check(got, x, rows, n_used, q, thresholds):
    """``got`` (numpy: total, quantile, above, mean, sd) against the rule on the values ``x`` [B, n_rows, V]."""
    ref = ensembles.weighted_reference(x, rows, n_used, q, PROBABILITIES, thresholds)
    assert np.array_equal(got["total"], ref["total"])
    assert np.array_equal(got["quantile"], ref["quantile"], equal_nan=True)
    assert np.array_equal(got["above"], ref["above"])
    assert np.array_equal(np.isnan(got["mean"]), np.isnan(ref["mean"])) and np.array_equal(np.isnan(got["sd"]), np.isnan(ref["sd"]))
    ld = ensembles.weighted_reference(x, rows, n_used, q, None, None, dtype=np.longdouble)
    worst = 0.0
    for b in range(x.shape[0]):
        m, W = int(n_used[b]), int(ref["total"][b])
        if W == 0:
            continue
        r, w = np.clip(rows[b, :m], 0, x.shape[1] - 1), q[b, :m].astype(np.longdouble)
        for v in range(x.shape[2]):
            if np.isnan(ref["mean"][b, v]):
                continue
            c = x[b, r, v].astype(np.longdouble)
            c = np.where(w > 0, c, 0.0)
            delta = (m + 2) * U * (w * np.abs(c)).sum() / W
            d = np.where(w > 0, c - ld["mean"][b, v], 0.0)
            bound = (m + 4) * U * (w * d * d).sum() / W + 2.0 * delta * (w * np.abs(d)).sum() / W + delta * delta
            err_mean = abs(np.longdouble(got["mean"][b, v]) - ld["mean"][b, v])
            err_var = abs(np.longdouble(got["sd"][b, v]) ** 2 - ld["sd"][b, v] ** 2)
            assert err_mean <= delta and err_var <= bound, (b, v, float(err_mean), float(delta), float(err_var), float(bound))
            worst = max(worst, float(err_mean / delta) if delta > 0 else 0.0, float(err_var / bound) if bound > 0 else 0.0)
    print("moments: used / bound at most %.3f" % worst)
    return ref


@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_plain_source_against_the_rule(n, V):
    rng = np.random.default_rng(1000 * n + V)
    n_rows = n + 3
    x = rng.choice(LEVELS, (B, n_rows, V))
    rows, n_used, q = _listed(rng, n, n_rows, V)
    thresholds = (float(LEVELS[2]), -0.5)                              # one equal to a value that is present
    dev = _dev()
    args = [torch.as_tensor(a).to(dev) for a in (x, rows, n_used, q)]
    got = _numpy(ensembles.series_weighted(*args, percentiles=PERCENTILES, thresholds=thresholds))
    ref = _check(got, x, rows, n_used, q, thresholds)
    assert np.all(ref["total"][n_used == 0] == 0) and (ref["above"] >= 0).all()
    again = _numpy(ensembles.series_weighted(*args, percentiles=PERCENTILES, thresholds=thresholds))      # a call repeats its bits
    assert all(np.array_equal(again[name].view(np.int64), got[name].view(np.int64)) for name in got)


def _device_values(ens, depth_edges):
    """log10 conductivity [B, n_slots, n_depth] as the device rasters it: gbp_ensemble_ranks' x_out with one segment of all the slots."""
    k = ens.k
    Bn, ns = k.shape
    z_np = ensembles.centres(depth_edges)
    z = torch.as_tensor(z_np).to(k.device)
    i32 = dict(dtype=torch.int32, device=k.device)
    out = ensembles._launch_ranks("gbp_ensemble_ranks", (Bn, ns, ens.edges.shape[2], k, ens.edges, ens.sigma, int(z_np.size), z), Bn, ns, int(z_np.size),
                                  k.device, torch.zeros((Bn, 1), **i32), torch.ones(Bn, **i32), torch.full((Bn,), ns, **i32), False, np.zeros(0), False,
                                  False, True)
    return out["x_out"].cpu().numpy()


def _random_ensemble(rng, ns, K):
    """B soundings of ns slots: k in 1 .. K, ascending interfaces in 0 .. 100 m, conductivities 10^level; slot 0 of every sounding empty."""
    k = rng.integers(1, K + 1, (B, ns)).astype(np.int32)
    k[:, 0] = 0
    edges, sigma = np.full((B, ns, K), np.inf), np.full((B, ns, K), np.nan)
    for b in range(B):
        for s in range(ns):
            kk = int(k[b, s])
            edges[b, s, :max(kk - 1, 0)] = np.sort(rng.uniform(0.0, 100.0, max(kk - 1, 0)))
            sigma[b, s, :kk] = 10.0 ** rng.choice(LEVELS, kk)
    return k, edges, sigma


@pytest.mark.parametrize("K", [1, 2, 64])
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_raster_source_against_the_rule(n, V, K):
    rng = np.random.default_rng(100000 * K + 1000 * n + V)
    ns = max(n + 3, 8)
    k, edges, sigma = _random_ensemble(rng, ns, K)
    rows, n_used, q = _listed(rng, n, ns - 1, V)
    rows = np.where((rows >= 0) & (rows < ns - 1), rows + 1, rows).astype(np.int32)      # the listed slots are filled ones
    for b in range(B):                                                 # a row of weight 0 may name the empty slot
        zero = np.nonzero(q[b, :n_used[b]] == 0)[0]
        if zero.size > 1:
            rows[b, zero[1]] = 0
    depth_edges = np.linspace(0.0, 100.0, V + 1)
    ens = _to_device(k, edges, sigma)
    x = _device_values(ens, depth_edges)
    assert np.isnan(x[:, 0]).all() and np.isfinite(x[:, 1:]).all()
    host = np.log10(ensembles.realisations_reference(k, edges, sigma, depth_edges))
    assert np.allclose(x[:, 1:], host[:, 1:], rtol=0, atol=4 * U * 3.0)
    thresholds = (float(x[0, rows[0, int(np.argmax(q[0, :n_used[0]]))], 0]), -1.5)      # a value that is present, and one between the levels
    dev = _dev()
    t_rows, t_nu, t_q = (torch.as_tensor(a).to(dev) for a in (rows, n_used, q))
    head = (B, ns, K, ens.k, ens.edges, ens.sigma, V, torch.as_tensor(ensembles.centres(depth_edges)).to(dev))
    call = lambda: _numpy(ensembles._launch_weighted("gbp_ensemble_weighted", head, B, V, dev, t_rows, t_nu, t_q, np.asarray(PROBABILITIES),      # noqa: E731
                                                     np.asarray(thresholds)))
    got = call()
    ref = _check(got, x, rows, n_used, q, thresholds)
    assert (ref["above"] >= 0).all() and np.any(ref["above"][0, 0] > 0)
    again = call()
    assert all(np.array_equal(again[name].view(np.int64), got[name].view(np.int64)) for name in got)


def _small_case(seed=3, n=65, V=5, K=4):
    rng = np.random.default_rng(seed)
    ns = n + 3
    k, edges, sigma = _random_ensemble(rng, ns, K)
    rows, n_used, q = _listed(rng, n, ns - 1, 3)
    rows = np.where((rows >= 0) & (rows < ns - 1), rows + 1, rows).astype(np.int32)
    return k, edges, sigma, rows, n_used, q, np.linspace(0.0, 100.0, V + 1)


def test_the_public_entry_blocks_and_derived_outputs():
    k, edges, sigma, rows, n_used, q, depth_edges = _small_case()
    n_used[1] = 7                                                      # (sounding 1 of the ragged list is empty: give it models)
    rows[1, :7], q[1, :7] = np.arange(1, 8), [3, 0, ONE, 1, 1, 0, 2]
    ens, dev = _to_device(k, edges, sigma), _dev()
    x = _device_values(ens, depth_edges)
    t_rows, t_nu, t_q = (torch.as_tensor(a).to(dev) for a in (rows, n_used, q))
    thresholds = (-1.0, 0.5)
    out = ensembles.weighted(ens, depth_edges, t_rows, t_q, n_used=t_nu, percentiles=PERCENTILES, thresholds=thresholds)
    o = _numpy(out)
    assert set(o) == {"mean", "sd", "exceedance", "weight_total", "n_effective"} | {"percentile_" + ensembles.percentile_name(p) for p in PERCENTILES}
    got = dict(total=o["weight_total"], quantile=np.stack([o["percentile_" + ensembles.percentile_name(p)] for p in PERCENTILES], axis=1),
               above=np.rint(o["exceedance"] * o["weight_total"][:, None, None].astype(np.float64)).astype(np.int64), mean=o["mean"], sd=o["sd"])
    ref = _check(got, x, rows, n_used, q, thresholds)
    assert np.array_equal(o["exceedance"], ref["above"] / ref["total"][:, None, None].astype(np.float64))
    live = np.arange(rows.shape[1])[None, :] < n_used[:, None]
    qf = np.where(live, q, 0).astype(np.float64)
    assert np.allclose(o["n_effective"], ref["total"].astype(np.float64) ** 2 / (qf * qf).sum(axis=1), rtol=1e-12, atol=0)      # (a sum of doubles)
    assert np.all(o["n_effective"] >= 1.0) and np.all(o["n_effective"] <= n_used)
    one = _numpy(ensembles.weighted(ens, depth_edges, t_rows, t_q, n_used=t_nu, percentiles=PERCENTILES, thresholds=thresholds, block=1))
    assert all(np.array_equal(one[name], o[name], equal_nan=True) for name in o)
    # float64 weights are quantised: the multiplicities over 2^40 as weights give the multiplicities back
    w = torch.as_tensor(np.where(live, q, 0) / float(ONE)).to(dev)
    fl = _numpy(ensembles.weighted(ens, depth_edges, t_rows, w, n_used=t_nu, percentiles=PERCENTILES, thresholds=thresholds))
    assert all(np.array_equal(fl[name], o[name], equal_nan=True) for name in o)
    # n_used = None: every listed row
    full_rows = torch.as_tensor(np.tile(np.arange(1, rows.shape[1] + 1, dtype=np.int32), (B, 1))).to(dev)
    every = _numpy(ensembles.weighted(ens, depth_edges, full_rows, torch.ones(rows.shape, dtype=torch.int64, device=dev), percentiles=(50,)))
    assert np.all(every["weight_total"] == rows.shape[1]) and np.all(every["n_effective"] == rows.shape[1])
    s = np.sort(x[:, 1:rows.shape[1] + 1], axis=1)
    assert np.array_equal(every["percentile_50"], s[:, max(int(np.ceil(0.5 * rows.shape[1])), 1) - 1])      # equal weights: the type-1 order statistic
    # quantise_weights on the device == numpy
    rng = np.random.default_rng(9)
    wr = rng.uniform(size=(5, 300)) ** 6
    nu = np.array([300, 0, 1, 17, 299])
    assert np.array_equal(ensembles.quantise_weights(torch.as_tensor(wr).to(dev), torch.as_tensor(nu).to(dev)).cpu().numpy(), ensembles.quantise_weights(wr, nu))


def test_zero_totals_and_non_finite_values():
    rng = np.random.default_rng(4)
    n, n_rows, V = 70, 80, 66
    x = rng.choice(LEVELS, (B, n_rows, V))
    rows = np.stack([rng.permutation(n_rows)[:n] for _ in range(B)]).astype(np.int32)
    n_used = np.array([n, n, n], dtype=np.int32)
    q = rng.integers(0, 4, (B, n)).astype(np.int64)
    q[1] = 0                                                           # W = 0 with rows listed
    x[0, rows[0, 3], 2], x[0, rows[0, 4], 65], x[2, rows[2, 5], 64] = np.nan, np.inf, -np.inf
    q[0, 3], q[0, 4], q[2, 5] = 2, 0, 1                                # the +inf has no weight: its column stays
    x[0, rows[0, 6], 7], q[0, 6] = np.nan, 0
    dev = _dev()
    got = _numpy(ensembles.series_weighted(*(torch.as_tensor(a).to(dev) for a in (x, rows, n_used, q)), percentiles=PERCENTILES, thresholds=(0.0,)))
    ref = _check(got, x, rows, n_used, q, (0.0,))
    assert np.isnan(got["quantile"][1]).all() and np.all(got["above"][1] == 0) and np.isnan(got["mean"][1]).all() and got["total"][1] == 0
    bad = np.zeros((B, V), dtype=bool)
    bad[0, 2], bad[2, 64] = True, True
    assert np.array_equal(got["above"][:, 0] == -1, bad) and np.array_equal(np.isnan(got["mean"]), bad | (np.arange(B) == 1)[:, None])
    assert np.array_equal(np.isnan(got["quantile"][:, 0]), np.isnan(ref["mean"]))
    # raster: a participating empty slot has the value NaN in every cell
    k, edges, sigma, rows, n_used, q, depth_edges = _small_case(seed=8)
    rows[0, 0], q[0, 0] = 0, 5
    ens = _to_device(k, edges, sigma)
    out = _numpy(ensembles.weighted(ens, depth_edges, *(torch.as_tensor(a).to(dev) for a in (rows, q)), n_used=torch.as_tensor(n_used).to(dev), thresholds=(0.0,)))
    assert np.isnan(out["mean"][0]).all() and np.isnan(out["percentile_50"][0]).all() and np.isnan(out["exceedance"][0]).all() and out["weight_total"][0] > 0
    assert np.isfinite(out["mean"][2]).all() and np.isfinite(out["exceedance"][2]).all()
    assert np.isnan(out["mean"][1]).all() and np.isnan(out["exceedance"][1]).all() and out["weight_total"][1] == 0 and np.isnan(out["n_effective"][1])


def test_skipped_outputs_and_the_refusals_of_both_entries():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(6)
    n, n_rows, V, K, n_p, n_t = 9, 12, 5, 4, 3, 2
    x = torch.as_tensor(rng.choice(LEVELS, (B, n_rows, V))).to(dev)
    k, edges, sigma = _random_ensemble(rng, n_rows, K)
    ens = _to_device(k, edges, sigma)
    z = torch.as_tensor(ensembles.centres(np.linspace(0.0, 100.0, V + 1))).to(dev)
    rows = torch.as_tensor(np.stack([rng.permutation(n_rows - 1)[:n] + 1 for _ in range(B)]).astype(np.int32)).to(dev)
    nu = torch.full((B,), n, dtype=torch.int32, device=dev)
    q = torch.as_tensor(rng.integers(0, 5, (B, n)).astype(np.int64)).to(dev)
    probs, thr = (ctypes.c_double * 16)(0.05, 0.5, 0.95), (ctypes.c_double * 8)(-1.0, 0.5)
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731

    def outputs():
        return dict(total=torch.full((B,), 7, dtype=torch.int64, device=dev), quantile=torch.full((B, n_p, V), 7.0, dtype=torch.float64, device=dev),
                    above=torch.full((B, n_t, V), 7, dtype=torch.int64, device=dev), stats=torch.full((B, 2, V), 7.0, dtype=torch.float64, device=dev))

    def series(o, B_=B, n_rows_=n_rows, V_=V, x_=x, n_=n, rows_=rows, nu_=nu, q_=q, n_p_=n_p, probs_=probs, n_t_=n_t, thr_=thr, skip=()):
        ptr = lambda name: None if name in skip else p(o[name])      # noqa: E731
        return lib.gbp_series_weighted(B_, n_rows_, V_, p(x_), n_, p(rows_), p(nu_), p(q_), n_p_, probs_, n_t_, thr_, ptr("total"), ptr("quantile"),
                                       ptr("above"), ptr("stats"), st)

    def raster(o, B_=B, ns_=n_rows, K_=K, k_=ens.k, e_=ens.edges, s_=ens.sigma, V_=V, z_=z, n_=n, rows_=rows, nu_=nu, q_=q, n_p_=n_p, probs_=probs, n_t_=n_t,
               thr_=thr, skip=()):
        ptr = lambda name: None if name in skip else p(o[name])      # noqa: E731
        return lib.gbp_ensemble_weighted(B_, ns_, K_, p(k_), p(e_), p(s_), V_, p(z_), n_, p(rows_), p(nu_), p(q_), n_p_, probs_, n_t_, thr_, ptr("total"),
                                         ptr("quantile"), ptr("above"), ptr("stats"), st)

    for entry, name in ((series, b"gbp_series_weighted"), (raster, b"gbp_ensemble_weighted")):
        full = outputs()
        assert entry(full) == 0, lib.gbp_last_error()
        torch.cuda.synchronize()
        assert not any(bool((v == 7).all()) for v in full.values())
        for skip in (("quantile",), ("above",), ("stats",), ("quantile", "above"), ("quantile", "above", "stats")):
            part = outputs()
            assert entry(part, skip=skip) == 0, lib.gbp_last_error()
            for key in part:                                           # a skipped output is not written, the others are unchanged
                assert bool((part[key] == 7).all()) if key in skip else torch.equal(part[key].view(torch.int64), full[key].view(torch.int64)), (skip, key)
        none = outputs()
        assert entry(none, n_p_=0, n_t_=0) == 0                        # nothing to write there: total and stats only
        assert bool((none["quantile"] == 7).all()) and bool((none["above"] == 7).all()) and torch.equal(none["total"], full["total"])
        assert torch.equal(none["stats"].view(torch.int64), full["stats"].view(torch.int64))
        untouched = outputs()
        nan_p, big_p, inf_t = (ctypes.c_double * 16)(0.5, float("nan")), (ctypes.c_double * 16)(1.5), (ctypes.c_double * 8)(float("inf"))
        bad = [dict(B_=-1), dict(V_=0), dict(n_=0), dict(n_=4097), dict(n_p_=-1), dict(n_p_=17), dict(n_t_=-1), dict(n_t_=9), dict(probs_=None), dict(thr_=None),
               dict(probs_=nan_p), dict(probs_=big_p), dict(thr_=inf_t), dict(rows_=None), dict(nu_=None), dict(q_=None), dict(skip=("total",)),
               dict(B_=2 ** 22, V_=64 * 2)]                           # 2^23 workgroups of 1024 threads
        bad += [dict(n_rows_=0), dict(x_=None)] if entry is series else [dict(ns_=0), dict(K_=0), dict(K_=65), dict(k_=None), dict(e_=None), dict(s_=None), dict(z_=None)]
        for kw in bad:
            assert entry(untouched, **kw) != 0 and name in lib.gbp_last_error(), kw
        assert entry(untouched, B_=0, rows_=None, q_=None) == 0        # an empty block: OK without a launch
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in untouched.values())   # nothing was written


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_the_planted_line_on_the_device():
    k, edges, sigma, x, y, truth = planted_line()
    S, n = k.shape
    ens, dev = _to_device(k, edges, sigma), _dev()
    products = dict(depth_edges=DEPTH_EDGES_LINE, percentiles=(5, 50, 95), thresholds=(-1.0,))
    plain = sections.sections(ens, x, y, Z1_LINE)
    out = sections.sections(ens, x, y, Z1_LINE, products=products)
    new = {"lateral_mean", "lateral_sd", "lateral_percentile_5", "lateral_percentile_50", "lateral_percentile_95", "lateral_exceedance"}
    assert set(plain) == {"state", "slot", "rows", "n_used", "section_k", "section_edges", "section_sigma", "step_distance", "log_score", "weight",
                          "chosen_weight", "n_effective", "log_partition"}                                  # without products: the keys of before
    assert set(out) == set(plain) | new
    assert all(torch.equal(out[name].view(torch.int64) if out[name].dtype == torch.float64 else out[name],
                           plain[name].view(torch.int64) if plain[name].dtype == torch.float64 else plain[name]) for name in plain)
    after = sections.lateral_products(ens, out, **products)
    direct = ensembles.weighted(ens, DEPTH_EDGES_LINE, out["rows"], out["weight"], n_used=out["n_used"], percentiles=(5, 50, 95), thresholds=(-1.0,))
    assert set(after) == new
    for name in new:
        assert torch.equal(after[name].view(torch.int64), out[name].view(torch.int64)), name
        assert torch.equal(direct[name[len("lateral_"):]].view(torch.int64), out[name].view(torch.int64)), name
    assert out["lateral_exceedance"].shape == (S, 1, 120) and out["lateral_mean"].shape == (S, 120)
    equal = ensembles.weighted(ens, DEPTH_EDGES_LINE, out["rows"], torch.ones((S, n), dtype=torch.int64, device=dev), percentiles=(50,))
    check_planted_products(equal["percentile_50"].cpu().numpy(), out["lateral_percentile_50"].cpu().numpy(), k, edges, sigma)
    o = _numpy(out)
    assert np.all(o["lateral_percentile_5"] <= o["lateral_percentile_50"]) and np.all(o["lateral_percentile_50"] <= o["lateral_percentile_95"])
    assert np.all((o["lateral_exceedance"] >= 0.0) & (o["lateral_exceedance"] <= 1.0)) and np.all(o["lateral_sd"] >= 0.0)
    # the device's weights through the rule, on the device's own values
    ref = ensembles.weighted_reference(_device_values(ens, DEPTH_EDGES_LINE), o["rows"], o["n_used"], ensembles.quantise_weights(o["weight"], o["n_used"]),
                                       [0.05, 0.5, 0.95], [-1.0])
    assert np.array_equal(o["lateral_percentile_50"], ref["quantile"][:, 1]) and np.array_equal(o["lateral_percentile_95"], ref["quantile"][:, 2])
    assert np.array_equal(o["lateral_exceedance"], ref["above"] / ref["total"][:, None, None].astype(np.float64))
    with pytest.raises(ValueError, match="marginals=True"):
        sections.sections(ens, x, y, Z1_LINE, marginals=False, products=products)


def test_the_command_line_writes_the_new_arrays(tmp_path):
    from geobipy_amd import survey
    res = survey.infer(os.path.join(GOLDEN, "resolve_options_small"), exact_jacobian=True, ensemble=16)
    path = str(tmp_path / "survey.npz")
    res.save(path)
    written = sections.load(sections.main([path, "--depth", "120", "--depth-axis", "60", "2", "--percentiles", "10", "50", "90", "--exceed", "-1.5", "-1"]))
    S = res["line"].size
    new = {"lateral_mean", "lateral_sd", "lateral_percentile_10", "lateral_percentile_50", "lateral_percentile_90", "lateral_exceedance"}
    assert new <= set(written) and written["lateral_mean"].shape == (S, 60) and written["lateral_exceedance"].shape == (S, 2, 60)
    direct = sections.from_survey(res, 120.0, products=dict(depth_edges=np.arange(61.0) * 2.0, percentiles=(10, 50, 90), thresholds=(-1.5, -1.0)))
    for name in new:
        assert np.array_equal(written[name], direct[name].cpu().numpy(), equal_nan=True), name
    has = written["state"] >= 0
    assert has.any() and np.isfinite(written["lateral_percentile_50"][has]).all() and np.isnan(written["lateral_mean"][~has]).all()
    assert np.all(written["lateral_exceedance"][has][:, 0] >= written["lateral_exceedance"][has][:, 1])      # a lower threshold is exceeded at least as often
    without = sections.load(sections.main([path, "--depth", "120"]))
    assert not (new & set(without)) and set(written) == set(without) | new
