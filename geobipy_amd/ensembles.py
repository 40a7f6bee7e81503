"""Posterior ensembles: the SAMPLED MODELS the device sampler keeps (``rjmcmc_gpu.DeviceChains(hitmap=True, ensemble=...)``;
csrc/gbp_rjmcmc.h ensemble_add; the host rule is ``inference.Posteriors(ensemble=...)`` / ``inference.ensemble_slots``).

A hit map is the one-dimensional shadow of the sampled models: it has lost the correlation between layers, so every functional of a
whole model -- a unit mean, a depth to a threshold, a prediction -- had to be requested before the chains ran.  The ensemble keeps
every ``thin``-th sampled model of every chain, in chain order, up to ``n_keep``; whatever was not foreseen is computed afterwards:

``realisations``   the kept models on a depth axis (gbp_ensemble_raster): joint realisations for a groundwater model, the correlation
                   between two depths, the conductance between two horizons picked afterwards ...
``rebin``          the hit map, the unit posteriors and the depths to a threshold of the kept models on axes, units and thresholds
                   chosen afterwards (gbp_ensemble_rebin: the sampler's own accumulators with weight 1); the outputs have the shapes
                   ``hitmap.products``, ``hitmap.interval_marginals`` and ``unit_posteriors.products`` take.

``diagnostics``    did the chain run long enough: per depth cell (and for the layer count and the misfit) the integrated
                   autocorrelation time, the effective sample size, the Monte-Carlo standard error of the posterior mean and a split
                   R-hat that works with one chain (gbp_ensemble_diagnostics / gbp_series_diagnostics).
                   ``python -m geobipy_amd.ensembles <ensemble.npz> --depth-axis N WIDTH`` writes them for a saved ensemble.

``correlation``    what is the vertical resolution: the posterior correlation between depth cells in a band R(c, c + j), j = 0 .. W, and
                   from it the thickness of the run of cells that move with a cell (``resolution_length``, metres) -- centred products on
                   the fp64 matrix cores, the series never written (gbp_ensemble_correlation / gbp_series_correlation / gbp_band_runs;
                   DESIGN.md 3.22).  ``python -m geobipy_amd.ensembles <ensemble.npz> --depth-axis N WIDTH --correlation [BAND]``.

``rank_diagnostics``  the same question for what the project publishes, the percentiles: rank-normalised and folded split R-hat, bulk
                   ESS, the ESS of the indicator I(x <= Q_p) behind every percentile and the tail ESS (Vehtari et al. 2021), built on the
                   rank of every kept sample within its (sounding, cell) column (gbp_ensemble_ranks / gbp_series_ranks; DESIGN.md
                   3.24); ``quantiles``: the exact sample quantiles of the kept models; ``correlation(rank=True)``: Spearman's.
                   ``python -m geobipy_amd.ensembles <ensemble.npz> --depth-axis N WIDTH --rank [--percentiles P ...]``.

``weighted``       every product above treats the kept models as equally weighted samples; this one takes weights -- the smoothed
                   marginals of ``sections.sections``, a borehole's likelihood, importance weights under another prior, dwell counts --
                   and gives, per depth cell, the weighted mean, sd, percentiles (type-1 inverse of the weighted ECDF) and exceedance
                   probabilities (gbp_ensemble_weighted / gbp_series_weighted).  The weights are INTEGER
                   multiplicities (``quantise_weights``: q = rint(w / max w * 2^40)), so the device is held to ``weighted_reference``
                   with ``==``.

There is no host fallback: all refuse tensors that are not on the device (``realisations_reference`` states the raster's rule in numpy,
``diagnostics_reference`` that of the diagnostics, ``correlation_reference`` and ``correlation_runs_reference`` those of the correlation, ``rank_counts_reference`` that of the ranks, ``weighted_reference`` that of the weighted products).
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._args import are_tensors, check_block, check_ensemble, on_device

Ensemble = namedtuple("Ensemble", ("k", "edges", "sigma", "misfit", "count", "thin", "log_mean_prior"))
Ensemble.__doc__ = """k int32 [B, n_keep] (0: empty slot), edges / sigma f64 [B, n_keep, K] (a slot's k - 1 interface depths then +inf,
its k conductivities then NaN), misfit f64 [B, n_keep] (chi^2), count [B] (filled slots: they are the first ``count`` ones of a
single chain), thin (every thin-th accumulated sample was kept), log_mean_prior f64 [B] (ln of the chain's prior mean conductivity)."""


def from_chains(dc):
    """The ``Ensemble`` of a sampler (``DeviceChains`` / ``TdemDeviceChains`` with ``ensemble=``, or ``replicates.Pooled`` of one:
    then [S, C n_keep, ...], the chains' ensembles one after the other, empty where a chain is not used), settled: the models the
    chains hold now have received the samples they were still owed."""
    if dc.t.get("ens_k") is None:
        raise ValueError("ensembles.from_chains: the chains kept no ensemble (DeviceChains(hitmap=True, ensemble=...))")
    k = dc.ens_k                                               # (attribute access settles the dwell times)
    t = dc.t
    return Ensemble(k, t["ens_edges"], t["ens_sigma"], t["ens_misfit"], (k > 0).sum(dim=1), int(dc.ensemble_thin), t["log_mean_prior"])


def _check(ens, what):
    for a in (ens.k, ens.edges, ens.sigma):
        if not torch.is_tensor(a) or a.device.type != "cuda":
            raise _lib.NativeLibraryError("ensembles.%s runs on the device (gbp_ensemble_%s); there is no host fallback" % (what[0], what[1]))
    k, edges, sigma, B, ne, K = check_ensemble(ens, slots="n_keep")
    if not 1 <= ne <= 4096 or not 1 <= K <= 64:
        raise ValueError("ensemble: n_keep must be in [1, 4096] and K in [1, 64]")
    return k, edges, sigma, B, ne, K


def centres(depth_edges):
    """Cell centres [n_depth] of ascending ``depth_edges`` [n_depth + 1] (numpy float64: 0.5 * (lower + upper))."""
    e = np.asarray(depth_edges, dtype=np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0.0):
        raise ValueError("depth_edges: at least two finite, ascending edges")
    return 0.5 * (e[:-1] + e[1:])


def check_slots(slots, n_keep):
    """``slots`` (None: all of them, in order) as an int32 numpy list of slot indices in [0, n_keep); repeats and any order are fine."""
    if slots is None:
        return np.arange(n_keep, dtype=np.int32)
    s = np.asarray(slots)
    if s.ndim != 1 or s.size < 1 or s.dtype.kind not in "iu":
        raise ValueError("slots: a list of at least one integer")
    if s.min() < 0 or s.max() >= n_keep:
        raise ValueError("slots: every index must lie in [0, %d)" % n_keep)
    return s.astype(np.int32)


def realisations(ens, depth_edges, slots=None, log10=True):
    """[B, R, n_depth] (torch, on the ensemble's device): the conductivity of slot ``slots[r]`` of every chain at the centre of every
    cell of ``depth_edges`` [n_depth + 1] -- that of the layer holding the centre, layer = #{l < k - 1 : edges[l] <= z} (the hit
    map's rule: an interface exactly at a centre gives the layer below).  ``log10=False``: the stored doubles bit for bit (S/m);
    ``log10=True``: their log10.  A row of NaN for an empty slot.  One gather kernel (gbp_ensemble_raster)."""
    k, edges, sigma, B, ne, K = _check(ens, ("realisations", "raster"))
    z_np = centres(depth_edges)
    s_np = check_slots(slots, ne)
    dev = k.device
    out = torch.empty((B, s_np.size, z_np.size), dtype=torch.float64, device=dev)
    if B > 0:
        z, s = torch.as_tensor(z_np).to(dev), torch.as_tensor(s_np).to(dev)
        _lib.call("gbp_ensemble_raster", dev, B, ne, K, k, edges, sigma, int(s_np.size), s, int(z_np.size), z, out)
    return torch.log10(out) if log10 else out


def realisations_reference(k, edges, sigma, depth_edges, slots=None):
    """The rule of ``realisations(..., log10=False)`` in numpy (host arrays): per chain and listed slot, ``sigma[searchsorted(edges[:k - 1],
    z, side="right")]`` at the cell centres z -- a row of NaN when k == 0."""
    k, edges, sigma = np.asarray(k), np.asarray(edges, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    z = centres(depth_edges)
    s = check_slots(slots, k.shape[1])
    out = np.full((k.shape[0], s.size, z.size), np.nan)
    for b in range(k.shape[0]):
        for r, q in enumerate(s):
            kk = int(k[b, q])
            if kk > 0:
                out[b, r] = sigma[b, q, np.searchsorted(edges[b, q, :kk - 1], z, side="right")]
    return out


def depth_axis(depth):
    """(n_depth, width) of the re-binning depth axis: ``depth`` = (n_depth, width), or uniform edges [n_depth + 1] starting at 0 (cell
    c spans [c, c + 1) width, the sampler's own axis)."""
    if isinstance(depth, tuple) and len(depth) == 2 and np.ndim(depth[0]) == 0 and np.ndim(depth[1]) == 0:
        n, w = depth
        if isinstance(n, bool) or int(n) != n:
            raise ValueError("depth axis: n_depth must be an integer")
        n, w = int(n), float(w)
    else:
        e = np.asarray(depth, dtype=np.float64).reshape(-1)
        if e.size < 2 or e[0] != 0.0:
            raise ValueError("depth axis: edges start at 0 (or give (n_depth, width))")
        n, w = e.size - 1, float(e[1] - e[0])
        if not np.all(np.isfinite(e)) or not np.allclose(np.diff(e), w, rtol=1e-9, atol=0.0):
            raise ValueError("depth axis: the edges must be uniform (the sampler's axis is)")
    if n < 1 or not (np.isfinite(w) and w > 0.0):
        raise ValueError("depth axis: n_depth >= 1 and a finite, positive width")
    return n, w


def rebin(ens, n_value_bins, value_half_width, depth, units=None, unit_kinds=("arithmetic", "harmonic"), first_above=(), first_below=(),
          surface=None, hitmap=True):
    """The posteriors of the kept models on axes chosen now: every filled slot counts once.  ``n_value_bins`` cells on
    +-``value_half_width`` decades about each chain's prior mean, ``depth`` = edges or (n_depth, width) (``depth_axis``); ``units`` as
    ``DeviceChains`` takes them (an interval spec, with ``surface`` [B] where it needs one, or bounds [M, 2] / [B, M, 2]), ``unit_kinds``,
    ``first_above`` / ``first_below`` likewise.  Returns {``hitmap`` int32 [B, n_value, n_depth] (unless ``hitmap=False``), ``unit_hist``
    int32 [B, Q, n_value, M], ``first_hist`` int32 [B, T, n_depth], ``first_none`` [B, T], and what ``unit_posteriors.products`` reads
    beside them: ``unit_z``, ``unit_kinds``, ``log_mean_prior``, ``value_half_width``, ``depth_bin_width``}.  The sampler's own
    accumulators do the binning (gbp_ensemble_rebin): on the sampler's axes, with thin = 1 and nothing dropped, the counts are the
    sampler's."""
    from .inference import check_first, check_unit_bounds, unit_kind_bits, unit_kind_names
    k, edges, sigma, B, ne, K = _check(ens, ("rebin", "rebin"))
    if isinstance(n_value_bins, bool) or int(n_value_bins) != n_value_bins or int(n_value_bins) < 1:
        raise ValueError("rebin: n_value_bins must be a positive integer")
    nv, hw = int(n_value_bins), float(value_half_width)
    if not (np.isfinite(hw) and hw > 0.0):
        raise ValueError("rebin: value_half_width must be finite and positive")
    nd, width = depth_axis(depth)
    dev = k.device
    lmp = torch.as_tensor(ens.log_mean_prior, dtype=torch.float64).to(dev).contiguous()
    if lmp.shape != (B,):
        raise ValueError("rebin: log_mean_prior [B]")
    bits, z = 0, None
    if units is not None:
        if isinstance(units, dict) or hasattr(units, "kind"):
            from .intervals import unit_bounds
            units = unit_bounds(units, B, surface=surface, max_depth=nd * width)
        z = check_unit_bounds(units)
        if z.ndim not in (2, 3) or (z.ndim == 3 and z.shape[0] != B):
            raise ValueError("units must be [M, 2] or [B, M, 2]")
        z = np.array(np.broadcast_to(z, (B,) + z.shape[-2:]))
        if not 1 <= z.shape[1] <= 16:
            raise ValueError("rebin: 1 .. 16 units")
        bits = unit_kind_bits(unit_kinds)
    kinds = unit_kind_names(bits)
    th, di = check_first(list(first_above) + list(first_below), [1] * len(first_above) + [-1] * len(first_below))
    M, Q, T = (0 if z is None else z.shape[1]), len(kinds), int(th.size)
    if not hitmap and M == 0 and T == 0:
        raise ValueError("rebin: nothing to compute (hitmap=False, no units, no thresholds)")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)      # noqa: E731  (the entry zeroes its outputs)
    out = dict(log_mean_prior=lmp, value_half_width=hw, depth_bin_width=width, unit_kinds=kinds)
    hm = i32(B, nv, nd) if hitmap else None
    uz = torch.as_tensor(z, dtype=torch.float64).to(dev).contiguous() if M else None
    uh, fh, fn = (i32(B, Q, nv, M) if M else None), (i32(B, T, nd) if T else None), (i32(B, T) if T else None)
    if B > 0:
        _lib.call("gbp_ensemble_rebin", dev, B, ne, K, k, edges, sigma, lmp, nv, hw, nd, width, hm, M, bits, uz, uh, T,
                  (ctypes.c_double * 4)(*(list(th) + [1.0] * (4 - T))), (ctypes.c_int32 * 4)(*([int(d) for d in di] + [1] * (4 - T))), fh, fn)
    for name, a in (("hitmap", hm), ("unit_z", uz), ("unit_hist", uh), ("first_hist", fh), ("first_none", fn)):
        if a is not None:
            out[name] = a
    return out


STAT_NAMES = ("mean", "sd", "rhat", "tau", "ess", "mcse")
MAX_LAG, MAX_SEGMENTS, MIN_CHAIN_COUNT = 255, 16, 8


def check_max_lag(max_lag):
    """``max_lag`` (None: 255) as an int in 1 .. 255."""
    if max_lag is None:
        return MAX_LAG
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 1 <= int(max_lag) <= MAX_LAG:
        raise ValueError("max_lag must be an integer in 1 .. %d" % MAX_LAG)
    return int(max_lag)


def lag_count(n, max_lag):
    """L of segments of length ``n`` (array or int): min(max_lag, n - 1), lowered by one if even, so lags 0 .. L form whole pairs."""
    L = np.minimum(int(max_lag), np.asarray(n, dtype=np.int64) - 1)
    return L - (1 - L % 2)


def diagnostics_reference(x, seg_start, n, max_lag, dtype=np.float64):
    """The rule of the chain diagnostics for one sounding, in numpy: ``x`` [n_rows, V], M = len(seg_start) segments of ``n`` rows each
    (segment m: rows seg_start[m] .. seg_start[m] + n - 1), evaluated in ``dtype``.  Returns {mean, sd, rhat, tau, ess, mcse [V], pairs
    int32 [V], rho [max_lag + 1, V] (NaN beyond L), pair_sums [(L + 1) / 2, V] (the P_k the walk compares with 0), L}.

    L = min(max_lag, n - 1), lowered by one if even.  Per variable, sums over a segment's rows: mean_m, d = x - mean_m, acov_m(l) =
    (1/n) sum_{t < n - l} d_t d_{t+l} (biased); W = (1/M) sum_m acov_m(0) n/(n-1); gm = (1/M) sum_m mean_m; Bn = sum_m (mean_m - gm)^2 /
    (M - 1) (0 when M = 1); vp = W (n-1)/n + Bn; rho_0 = 1, rho_l = 1 - (W - (1/M) sum_m acov_m(l) n/(n-1)) / vp.  Geyer's initial
    monotone sequence on the pairs P_k = rho_2k + rho_2k+1: S = prev = P_0, pairs = 1; for k = 1, 2, ...: stop unless P_k > 0, else
    prev = min(prev, P_k), S += prev, pairs += 1.  tau = max(2 S - 1, 1 / log10(M n)), ess = M n / tau, rhat = sqrt(vp / W), sd =
    sqrt(vp), mcse = sqrt(vp / ess), mean = gm; pairs == (L + 1) / 2: the sum ran into the lag cap.  M == 0 or n < 4: everything NaN,
    pairs 0.  A variable whose used samples are all one value (compared as stored): mean = it, sd = 0, the rest NaN, pairs 0; one with
    a non-finite used sample: all NaN, pairs 0."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("diagnostics_reference: x [n_rows, V]")
    max_lag = check_max_lag(max_lag)
    starts = [int(q) for q in np.asarray(seg_start).reshape(-1)]
    M, N, V = len(starts), int(n), x.shape[1]
    if M > MAX_SEGMENTS:
        raise ValueError("diagnostics_reference: at most %d segments" % MAX_SEGMENTS)
    out = {name: np.full(V, np.nan, dtype=dtype) for name in STAT_NAMES}
    out.update(pairs=np.zeros(V, dtype=np.int32), rho=np.full((max_lag + 1, V), np.nan, dtype=dtype), pair_sums=np.zeros((0, V), dtype=dtype), L=0)
    if M == 0 or N < 4:
        return out
    if min(starts) < 0 or max(starts) + N > x.shape[0]:
        raise ValueError("diagnostics_reference: a segment leaves the rows 0 .. %d" % (x.shape[0] - 1))
    L = int(lag_count(N, max_lag))
    stored = np.stack([x[q:q + N] for q in starts])                    # [M, N, V]
    xs = stored.astype(dtype)
    Nf, Mf, one = dtype(N), dtype(M), dtype(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean_m = xs.sum(axis=1) / Nf                                   # [M, V]
        d = xs - mean_m[:, None, :]
        acov = np.stack([(d[:, :N - l] * d[:, l:]).sum(axis=1) / Nf for l in range(L + 1)], axis=1)    # [M, L + 1, V]
        bessel = Nf / (Nf - one)
        A = acov.sum(axis=0) / Mf * bessel                             # [L + 1, V]
        W = A[0]
        gm = mean_m.sum(axis=0) / Mf
        Bn = ((mean_m - gm) ** 2).sum(axis=0) / (Mf - one) if M > 1 else np.zeros(V, dtype=dtype)
        vp = W * (Nf - one) / Nf + Bn
        rho = one - (W - A) / vp
        rho[0] = one
        P = rho[0::2] + rho[1::2]                                      # [(L + 1) / 2, V]
        S, prev = P[0].copy(), P[0].copy()
        pairs, open_ = np.ones(V, dtype=np.int32), np.ones(V, dtype=bool)
        for k in range(1, P.shape[0]):
            open_ &= P[k] > 0
            prev = np.where(open_, np.minimum(prev, P[k]), prev)
            S = np.where(open_, S + prev, S)
            pairs += open_
        total = Mf * Nf
        tau = np.maximum(dtype(2) * S - one, one / np.log10(total))
        ess = total / tau
        stats = dict(mean=gm, sd=np.sqrt(vp), rhat=np.sqrt(vp / W), tau=tau, ess=ess, mcse=np.sqrt(vp / ess))
    flat = stored.reshape(M * N, V)
    bad = ~np.all(np.isfinite(flat), axis=0)
    with np.errstate(invalid="ignore"):
        const = ~bad & (flat.min(axis=0) == flat.max(axis=0))
    for name in STAT_NAMES:
        a = np.array(stats[name], dtype=dtype)
        a[bad | const] = np.nan
        out[name] = a
    out["mean"][const] = flat[0, const].astype(dtype)
    out["sd"][const] = 0
    pairs[bad | const] = 0
    rho[:, bad | const] = np.nan
    out["pairs"], out["pair_sums"], out["L"] = pairs, P, L
    out["rho"][:L + 1] = rho
    return out


def segments(count_per_chain, slots_per_chain):
    """Split-chain segments from the filled-slot counts [B, C] of C chains whose ensembles lie one after the other, ``slots_per_chain``
    slots each (the chains' filled slots are their first ones).  Chains with fewer than 8 filled slots are left out; with C_used >= 1
    chains left n = min count, N = n // 2, M = 2 C_used, and chain c gives the segments that start at its slots 0 and N (an odd n
    leaves the last slot unused).  Returns numpy (seg_start int32 [B, 2 C], seg_m int32 [B], seg_n int32 [B], n_chains_used int32 [B]);
    C_used == 0: M = N = 0."""
    cnt = np.asarray(count_per_chain)
    if cnt.ndim != 2 or cnt.shape[1] < 1 or cnt.dtype.kind not in "iu":
        raise ValueError("segments: integer counts [B, C]")
    B, C = cnt.shape
    per = int(slots_per_chain)
    if per < 1 or 2 * C > MAX_SEGMENTS:
        raise ValueError("segments: slots_per_chain >= 1 and at most %d chains" % (MAX_SEGMENTS // 2))
    if cnt.size and (cnt.min() < 0 or cnt.max() > per):
        raise ValueError("segments: every count must lie in 0 .. slots_per_chain")
    used = cnt >= MIN_CHAIN_COUNT
    n_used = used.sum(axis=1).astype(np.int32)
    n = np.where(used, cnt, np.iinfo(np.int64).max).min(axis=1, initial=np.iinfo(np.int64).max)
    N = np.where(n_used > 0, n // 2, 0).astype(np.int32)
    start = np.zeros((B, 2 * C), dtype=np.int32)
    for b in range(B):
        chains = np.nonzero(used[b])[0]
        start[b, 0:2 * chains.size:2] = chains * per
        start[b, 1:2 * chains.size:2] = chains * per + N[b]
    return start, (2 * n_used).astype(np.int32), N, n_used


def _check_segments(seg_start, seg_m, seg_n, B, n_rows, what):
    """dtype, shapes and values of a caller's segment lists (the kernel reads seg_start[b, :seg_m[b]] and the rows they name: these
    checks are what keeps it inside its arrays); any device."""
    for a in (seg_start, seg_m, seg_n):
        if a.dtype != torch.int32:
            raise TypeError("%s: seg_start, seg_m and seg_n are int32" % what)
    if seg_start.ndim != 2 or seg_start.shape[0] != B or not 1 <= seg_start.shape[1] <= MAX_SEGMENTS or seg_m.shape != (B,) or seg_n.shape != (B,):
        raise ValueError("%s: seg_start [B, M_max] with 1 <= M_max <= %d, seg_m and seg_n [B]" % (what, MAX_SEGMENTS))
    if not (seg_start.device == seg_m.device == seg_n.device):
        raise ValueError("%s: seg_start, seg_m and seg_n live on one device" % what)
    if B > 0:
        M_max = seg_start.shape[1]
        live = torch.arange(M_max, device=seg_start.device)[None, :] < seg_m[:, None]
        ok = (seg_m >= 0).all() & (seg_m <= M_max).all() & (seg_n >= 0).all() & (~live | ((seg_start >= 0) & (seg_start + seg_n[:, None] <= n_rows))).all()
        if not bool(ok):
            raise ValueError("%s: a segment leaves the rows 0 .. %d (or seg_m is outside 0 .. M_max)" % (what, n_rows - 1))
    return seg_start.contiguous(), seg_m.contiguous(), seg_n.contiguous()


def _check_series(x, seg_start, seg_m, seg_n, what, entry, check_v=lambda V: None, ranked=False):
    """The checks ``series_diagnostics`` and ``series_correlation`` share, in their order: tensors, x, ``check_v(V)`` (the entry's own
    check that needs V), the segment lists, and the device last.  Returns x and the lists, contiguous, and what ``check_v`` gave.
    ``ranked``: the columns are ranked too (``series_ranks``): at most 16 384 rows, and segments that do not overlap."""
    are_tensors((x, seg_start, seg_m, seg_n), "ensembles", what, entry)
    if x.dtype != torch.float64:
        raise TypeError("%s: x is float64" % what)
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[1] > 32768:
        raise ValueError("%s: x is float64 [B, n_rows, V] with 1 <= n_rows <= 32768 and V >= 1" % what)
    if ranked and x.shape[1] > RANK_MAX_ROWS:
        raise ValueError("%s: at most %d rows where columns are ranked (a padded column lives in LDS); x has %d" % (what, RANK_MAX_ROWS, x.shape[1]))
    own = check_v(x.shape[2])
    seg_start, seg_m, seg_n = _check_segments(seg_start, seg_m, seg_n, x.shape[0], x.shape[1], what)
    if ranked and seg_m.numel() and bool((seg_m.to(torch.int64) * seg_n.to(torch.int64) > x.shape[1]).any()):
        raise ValueError("%s: the segments overlap (seg_m * seg_n > n_rows)" % what)
    on_device((x, seg_start, seg_m, seg_n), "ensembles", what, entry)
    return x.contiguous(), seg_start, seg_m, seg_n, own


def _unpack(stats, pairs, rho, seg_n, max_lag):
    out = {name: stats[:, i] for i, name in enumerate(STAT_NAMES)}
    L = torch.clamp(seg_n.to(torch.int64) - 1, max=max_lag)
    L = L - (1 - L % 2)
    out["pairs"] = pairs
    out["truncated"] = (pairs > 0) & (pairs == ((L + 1) // 2)[:, None])
    if rho is not None:
        out["rho"] = rho
    return out


def series_diagnostics(x, seg_start, seg_m, seg_n, max_lag=255, return_rho=False):
    """The chain diagnostics (``diagnostics_reference`` states the rule) of the series ``x`` f64 [B, n_rows, V] on the device: sounding
    b has seg_m[b] segments of seg_n[b] rows that start at seg_start[b, :seg_m[b]] (int32 device tensors, [B, M_max] and [B]).  Returns
    {mean, sd, rhat, tau, ess, mcse f64 [B, V], pairs int32 [B, V], truncated bool [B, V] (the sum ran into the lag cap: ess is an
    over-estimate)} and, with ``return_rho``, rho f64 [B, max_lag + 1, V].  One kernel (gbp_series_diagnostics)."""
    max_lag = check_max_lag(max_lag)
    x, seg_start, seg_m, seg_n, _ = _check_series(x, seg_start, seg_m, seg_n, "series_diagnostics", "gbp_series_diagnostics")
    (B, n_rows, V), dev = x.shape, x.device
    stats = torch.empty((B, 6, V), dtype=torch.float64, device=dev)
    pairs = torch.empty((B, V), dtype=torch.int32, device=dev)
    rho = torch.empty((B, max_lag + 1, V), dtype=torch.float64, device=dev) if return_rho else None
    if B > 0:
        _lib.call("gbp_series_diagnostics", dev, B, n_rows, V, x, int(seg_start.shape[1]), seg_start, seg_m, seg_n, max_lag, stats, pairs, rho)
    return _unpack(stats, pairs, rho, seg_n, max_lag)


def check_chains(chains, n_slots):
    """``chains`` as an int in 1 .. 8 that divides the slot axis."""
    if isinstance(chains, bool) or not isinstance(chains, (int, np.integer)) or not 1 <= int(chains) <= MAX_SEGMENTS // 2:
        raise ValueError("chains must be an integer in 1 .. %d" % (MAX_SEGMENTS // 2))
    if n_slots % int(chains) != 0:
        raise ValueError("chains = %d does not divide the slot axis (%d slots)" % (int(chains), n_slots))
    return int(chains)


def _check_chained(ens, chains, what, entry, misfit):
    """What ``diagnostics`` and ``correlation`` ask of an ensemble whose slot axis holds ``chains`` chains (``misfit``: it takes part),
    refused in this order: tensors, shapes, dtypes, sizes, and the device last.  Returns k, edges, sigma (contiguous), B, n_slots, K,
    C, the lists of ``segments`` for the chains' filled slots on the device (seg_start, seg_m, seg_n) and n_chains_used."""
    tensors = (ens.k, ens.edges, ens.sigma, ens.misfit) if misfit else (ens.k, ens.edges, ens.sigma)
    are_tensors(tensors, "ensembles", what, entry)
    k, edges, sigma, B, ns, K = check_ensemble(ens, misfit=misfit)
    C = check_chains(chains, ns)
    if not 1 <= ns <= 4096 * C or not 1 <= K <= 64:
        raise ValueError("ensemble: at most 4096 slots per chain and K in [1, 64]")
    on_device(tensors, "ensembles", what, entry)
    dev = k.device
    count = (k.reshape(B, C, ns // C) > 0).sum(dim=2).cpu().numpy()
    start, seg_m, seg_n, used = (torch.as_tensor(a).to(dev) for a in segments(count, ns // C))
    return k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used


def diagnostics(ens, depth_edges, chains=1, max_lag=None, block=None, return_rho=False):
    """Did the chains run long enough?  Per sounding and cell of ``depth_edges`` [n_depth + 1] the diagnostics of the series log10
    conductivity at the cell centre over the kept models (``diagnostics_reference`` states the rule, ``segments`` the split of every
    chain into two halves; ``chains`` = C: the slot axis holds C chains' ensembles one after the other, as ``replicates.Pooled`` yields
    them), the series never written to memory (gbp_ensemble_diagnostics).  Returns mean, sd, rhat, tau, ess, mcse f64 [B, n_depth],
    pairs int32 and truncated bool [B, n_depth], tau_iterations = tau * ens.thin; the same names with the suffixes ``_k`` (the layer
    count) and ``_misfit`` (log10 of the misfit) [B]; n_chains_used, segment_length, n_segments int32 [B]; ess_min [B], the smallest
    finite ess over the cells (NaN: none); with ``return_rho`` rho [B, max_lag + 1, n_depth].  ``block``: soundings per launch (None:
    all).  A cell no interface reached is constant: sd = 0, the rest NaN."""
    max_lag = check_max_lag(max_lag)
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    check_block(block, "diagnostics")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "diagnostics", "gbp_ensemble_diagnostics", misfit=True)
    nd, dev = int(z_np.size), k.device
    stats = torch.empty((B, 6, nd), dtype=torch.float64, device=dev)
    pairs = torch.empty((B, nd), dtype=torch.int32, device=dev)
    rho = torch.empty((B, max_lag + 1, nd), dtype=torch.float64, device=dev) if return_rho else None
    if B > 0:
        z = torch.as_tensor(z_np).to(dev)
        step = B if block is None else int(block)
        for b0 in range(0, B, step):
            s = slice(b0, min(B, b0 + step))
            _lib.call("gbp_ensemble_diagnostics", dev, s.stop - s.start, ns, K, k[s], edges[s], sigma[s], nd, z, 2 * C, start[s], seg_m[s], seg_n[s],
                      max_lag, stats[s], pairs[s], None if rho is None else rho[s])
    out = _unpack(stats, pairs, rho, seg_n, max_lag)
    scalars = torch.stack((k.to(torch.float64), torch.log10(ens.misfit.to(torch.float64))), dim=2)
    two = series_diagnostics(scalars, start, seg_m, seg_n, max_lag=max_lag)
    for name in STAT_NAMES + ("pairs", "truncated"):
        out[name + "_k"], out[name + "_misfit"] = two[name][:, 0], two[name][:, 1]
    thin = int(ens.thin)
    out["tau_iterations"], out["tau_iterations_k"], out["tau_iterations_misfit"] = out["tau"] * thin, out["tau_k"] * thin, out["tau_misfit"] * thin
    out["n_chains_used"], out["segment_length"], out["n_segments"] = used, seg_n, seg_m
    ess = out["ess"]
    lowest = torch.where(torch.isfinite(ess), ess, torch.full_like(ess, float("inf"))).min(dim=1).values if nd else torch.full((B,), float("inf"), device=dev)
    out["ess_min"] = torch.where(torch.isfinite(lowest), lowest, torch.full_like(lowest, float("nan")))
    return out


RANK_MAX_ROWS, RANK_MAX_PROBABILITIES, RANK_BLOCK_BYTES = 16384, 16, 2 << 30


def check_probabilities(probabilities):
    """``probabilities`` (None: none) as a float64 numpy list of at most 16 finite numbers in [0, 1]."""
    if probabilities is None:
        return np.zeros(0, dtype=np.float64)
    p = np.asarray(probabilities, dtype=np.float64)
    if p.ndim != 1 or p.size > RANK_MAX_PROBABILITIES:
        raise ValueError("probabilities: a list of at most %d numbers" % RANK_MAX_PROBABILITIES)
    if not np.all(np.isfinite(p) & (p >= 0.0) & (p <= 1.0)):
        raise ValueError("probabilities: every one finite and in [0, 1]")
    return p


def check_percentiles(percentiles):
    """``percentiles`` as a tuple of 1 .. 16 distinct, ascending floats in [0, 100]."""
    try:
        q = np.asarray(percentiles, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("percentiles: a list of numbers in [0, 100]")
    if q.ndim != 1 or not 1 <= q.size <= RANK_MAX_PROBABILITIES:
        raise ValueError("percentiles: a list of 1 .. %d numbers" % RANK_MAX_PROBABILITIES)
    if not np.all(np.isfinite(q) & (q >= 0.0) & (q <= 100.0)) or not np.all(np.diff(q) > 0.0):
        raise ValueError("percentiles: distinct, ascending numbers in [0, 100]")
    return tuple(float(v) for v in q)


def percentile_name(q):
    """'5' for 5.0, '2.5' for 2.5: what follows ``ess_percentile_`` and ``quantile_``."""
    return "%g" % q


def rank_counts_reference(x, seg_start, n, fold=False, probabilities=None):
    """The rule of the ranks for one sounding, in numpy: ``x`` [n_rows, V], M = len(seg_start) segments of ``n`` rows each (the lists
    ``segments`` builds); the used rows are r_j = seg_start[m] + t, j = m n + t, nu = M n of them.  Returns {less, leq int32
    [n_rows, V], order f64 [Q, 2, V]} for Q = len(probabilities) <= 16 probabilities in [0, 1].

    Per variable v with the column c_j = x[r_j, v] and s = c sorted ascending: lo_i = floor((nu - 1) p_i) (one fp64 product),
    order[i, 0, v] = s[lo_i], order[i, 1, v] = s[min(lo_i + 1, nu - 1)] -- before any folding.  ``fold``: med = 0.5 (s[(nu - 1) // 2] +
    s[nu // 2]), c_j <- |c_j - med| (one subtraction, then the absolute value; +inf ranks as the largest).  less[r_j] = #{i : c_i < c_j},
    leq[r_j] = #{i : c_i <= c_j}: values compare as doubles (-0.0 equals +0.0), so 0 <= less < leq <= nu.  A row in no segment:
    less = leq = -1.  M == 0 or n < 4: -1 everywhere and order NaN.  A variable with a non-finite used value: -1 at the used rows
    too, its order NaN.  Segments that overlap (M n > n_rows) are refused."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("rank_counts_reference: x [n_rows, V]")
    p = check_probabilities(probabilities)
    starts = [int(q) for q in np.asarray(seg_start).reshape(-1)]
    M, N, V = len(starts), int(n), x.shape[1]
    if M > MAX_SEGMENTS:
        raise ValueError("rank_counts_reference: at most %d segments" % MAX_SEGMENTS)
    less, leq = np.full(x.shape, -1, dtype=np.int32), np.full(x.shape, -1, dtype=np.int32)
    order = np.full((p.size, 2, V), np.nan)
    out = dict(less=less, leq=leq, order=order)
    if M == 0 or N < 4:
        return out
    if min(starts) < 0 or max(starts) + N > x.shape[0]:
        raise ValueError("rank_counts_reference: a segment leaves the rows 0 .. %d" % (x.shape[0] - 1))
    nu = M * N
    if nu > x.shape[0]:
        raise ValueError("rank_counts_reference: the segments overlap (M n > n_rows)")
    rows = np.concatenate([np.arange(q, q + N) for q in starts])
    lo = np.floor(np.float64(nu - 1) * p).astype(np.int64)
    for v in range(V):
        c = x[rows, v]
        if not np.all(np.isfinite(c)):
            continue
        s = np.sort(c)
        order[:, 0, v], order[:, 1, v] = s[lo], s[np.minimum(lo + 1, nu - 1)]
        if fold:
            with np.errstate(over="ignore"):
                med = 0.5 * (s[(nu - 1) // 2] + s[nu // 2])
                c = np.abs(c - med)
            s = np.sort(c)
        less[rows, v], leq[rows, v] = np.searchsorted(s, c, side="left"), np.searchsorted(s, c, side="right")
    return out


def _used_count(seg_m, seg_n, like):
    """nu = M N per sounding as f64 shaped to broadcast against ``like`` [B, ...] (torch)."""
    nu = seg_m.to(torch.float64) * seg_n.to(torch.float64)
    return nu.reshape((-1,) + (1,) * (like.ndim - 1))


def midranks(less, leq):
    """(less + leq + 1) / 2 in f64 -- ``scipy.stats.rankdata(method="average")`` of the column; NaN where less < 0.  Torch."""
    r = less.to(torch.float64)                                         # (in place: one f64 series beside the counts)
    r += leq
    r += 1.0
    r /= 2.0
    return r.masked_fill_(less < 0, float("nan"))


def normal_scores(less, leq, nu):
    """z = ndtri((r - 3/8) / (nu + 1/4)) of the midrank r (Blom's scores); nu broadcasts against less; NaN where less < 0.  Torch."""
    r = midranks(less, leq)
    r -= 0.375
    r /= nu + 0.25
    return torch.special.ndtri(r, out=r)


def quantile_cells(nu, p):
    """lo = floor((nu - 1) p) and g = (nu - 1) p - lo (f64 torch, shaped as nu): the cell of numpy's ``method="linear"``."""
    h = (nu - 1.0) * float(p)
    lo = torch.floor(h)
    return lo, h - lo


def indicators(less, nu, p):
    """I_p = 1.0 where less <= floor((nu - 1) p), else 0.0 -- with ties exactly I(x <= Q_p).  Torch, f64."""
    return (less.to(torch.float64) <= quantile_cells(nu, p)[0]).to(torch.float64)


def sample_quantile(order, nu, i, p):
    """order[..., i, 0, :] + g (order[..., i, 1, :] - order[..., i, 0, :]): numpy's ``method="linear"`` quantile.  Torch."""
    o0, o1 = order[..., i, 0, :], order[..., i, 1, :]
    g = quantile_cells(nu, p)[1]
    return o0 + g.reshape(g.shape[:o0.ndim]) * (o1 - o0)


def _truncated(pairs, L):
    return (pairs > 0) & (pairs == (L + 1) // 2)


def rank_products_reference(z, z_folded, indicator, seg_start, n, max_lag, dtype=np.float64):
    """The rank products of one sounding from its derived series (numpy [n_rows, V]; ``indicator``: {percentile: series}), each
    through ``diagnostics_reference`` in ``dtype``: rhat_bulk, ess_bulk, tau_bulk, truncated_bulk (z), rhat_folded (z_folded),
    rhat_rank = max of the two, ess_percentile_<p> (I_p), ess_tail = min of the ESS of the lowest and the highest percentile; NaN
    propagates through max and min."""
    d = diagnostics_reference(z, seg_start, n, max_lag, dtype=dtype)
    out = dict(rhat_bulk=d["rhat"], ess_bulk=d["ess"], tau_bulk=d["tau"], truncated_bulk=_truncated(d["pairs"], d["L"]))
    out["rhat_folded"] = diagnostics_reference(z_folded, seg_start, n, max_lag, dtype=dtype)["rhat"]
    out["rhat_rank"] = np.maximum(out["rhat_bulk"], out["rhat_folded"])
    qs = sorted(indicator)
    for q in qs:
        out["ess_percentile_" + percentile_name(q)] = diagnostics_reference(indicator[q], seg_start, n, max_lag, dtype=dtype)["ess"]
    out["ess_tail"] = np.minimum(out["ess_percentile_" + percentile_name(qs[0])], out["ess_percentile_" + percentile_name(qs[-1])])
    return out


def rank_diagnostics_reference(x, seg_start, n, max_lag, percentiles=(5, 50, 95), dtype=np.float64):
    """The rule of the rank diagnostics for one sounding on the host: ``rank_counts_reference`` (unfolded with p = percentiles / 100,
    and folded), the derived series by the expressions the device uses (``normal_scores``, ``indicators``, ``sample_quantile``, here
    on CPU tensors), then ``rank_products_reference``; adds quantile_<p> [V]."""
    qs = check_percentiles(percentiles)
    x = np.asarray(x, dtype=np.float64)
    starts = np.asarray(seg_start).reshape(-1)
    plain = rank_counts_reference(x, starts, n, fold=False, probabilities=[q / 100.0 for q in qs])
    folded = rank_counts_reference(x, starts, n, fold=True)
    nu = torch.tensor(float(len(starts) * int(n)), dtype=torch.float64)
    t = lambda a: torch.as_tensor(a)      # noqa: E731
    z = normal_scores(t(plain["less"]), t(plain["leq"]), nu).numpy()
    zf = normal_scores(t(folded["less"]), t(folded["leq"]), nu).numpy()
    ind = {q: indicators(t(plain["less"]), nu, q / 100.0).numpy() for q in qs}
    out = rank_products_reference(z, zf, ind, starts, n, max_lag, dtype=dtype)
    for i, q in enumerate(qs):
        out["quantile_" + percentile_name(q)] = sample_quantile(t(plain["order"]), nu, i, q / 100.0).numpy()
    return out


def _launch_ranks(entry, head, B, n_rows, V, dev, seg_start, seg_m, seg_n, fold, p, counts, order, values):
    """One call of gbp_series_ranks / gbp_ensemble_ranks (``head``: the entry's arguments up to M_max) on fresh outputs: {less, leq
    int32 [B, n_rows, V] (``counts``), order f64 [B, Q, 2, V] (``order``), x_out f64 [B, n_rows, V] (``values``)}."""
    out = {}
    if counts:
        out["less"], out["leq"] = (torch.empty((B, n_rows, V), dtype=torch.int32, device=dev) for _ in range(2))
    if order:
        out["order"] = torch.empty((B, p.size, 2, V), dtype=torch.float64, device=dev)
    if values:
        out["x_out"] = torch.empty((B, n_rows, V), dtype=torch.float64, device=dev)
    given = lambda name: out[name] if name in out and out[name].numel() else None      # noqa: E731
    if B > 0:
        _lib.call(entry, dev, *head, int(seg_start.shape[1]), seg_start, seg_m, seg_n, int(bool(fold)), int(p.size),
                  (ctypes.c_double * max(int(p.size), 1))(*p), given("less"), given("leq"), given("order"), given("x_out"))
    return out


def series_ranks(x, seg_start, seg_m, seg_n, fold=False, probabilities=None, counts=True, values=False):
    """The ranks (``rank_counts_reference`` states the rule) within the columns of the series ``x`` f64 [B, n_rows, V] on the device,
    n_rows <= 16 384, segments as ``series_diagnostics`` takes them (they may not overlap).  Returns {less, leq int32 [B, n_rows, V]
    (``counts``), order f64 [B, Q, 2, V] (with ``probabilities``), x_out f64 [B, n_rows, V] (``values``: the ranked values at the used
    rows, NaN elsewhere)}.  One kernel (gbp_series_ranks)."""
    p = check_probabilities(probabilities)
    x, seg_start, seg_m, seg_n, _ = _check_series(x, seg_start, seg_m, seg_n, "series_ranks", "gbp_series_ranks", ranked=True)
    B, n_rows, V = x.shape
    return _launch_ranks("gbp_series_ranks", (B, n_rows, V, x), B, n_rows, V, x.device, seg_start, seg_m, seg_n, fold, p, counts,
                         p.size > 0, values)


def _rank_products(ranker, seg_start, seg_m, seg_n, max_lag, qs):
    """The products of ``rank_products_reference`` and the quantiles on the device: ``ranker(fold, p)`` gives {less, leq, order} of
    the series; the derived series exist one at a time."""
    p = np.asarray([q / 100.0 for q in qs], dtype=np.float64)
    r = ranker(False, p)
    less = r["less"]
    nu = _used_count(seg_m, seg_n, less)
    d = series_diagnostics(normal_scores(less, r["leq"], nu), seg_start, seg_m, seg_n, max_lag=max_lag)
    out = dict(rhat_bulk=d["rhat"], ess_bulk=d["ess"], tau_bulk=d["tau"], truncated_bulk=d["truncated"])
    for i, q in enumerate(qs):
        out["ess_percentile_" + percentile_name(q)] = series_diagnostics(indicators(less, nu, p[i]), seg_start, seg_m, seg_n, max_lag=max_lag)["ess"]
        out["quantile_" + percentile_name(q)] = sample_quantile(r["order"], nu, i, p[i])
    del r, less, d
    f = ranker(True, np.zeros(0))
    out["rhat_folded"] = series_diagnostics(normal_scores(f["less"], f["leq"], nu), seg_start, seg_m, seg_n, max_lag=max_lag)["rhat"]
    out["rhat_rank"] = torch.maximum(out["rhat_bulk"], out["rhat_folded"])
    out["ess_tail"] = torch.minimum(out["ess_percentile_" + percentile_name(qs[0])], out["ess_percentile_" + percentile_name(qs[-1])])
    return out


def series_rank_diagnostics(x, seg_start, seg_m, seg_n, max_lag=255, percentiles=(5, 50, 95)):
    """The rank diagnostics (``rank_diagnostics_reference`` states the rule) of the series ``x`` f64 [B, n_rows, V] on the device:
    rhat_bulk, ess_bulk, tau_bulk, rhat_folded, rhat_rank, ess_percentile_<p>, ess_tail, quantile_<p> f64 [B, V], truncated_bulk bool
    [B, V].  gbp_series_ranks twice (unfolded, folded), the derived series through gbp_series_diagnostics."""
    max_lag = check_max_lag(max_lag)
    qs = check_percentiles(percentiles)
    x, seg_start, seg_m, seg_n, _ = _check_series(x, seg_start, seg_m, seg_n, "series_rank_diagnostics", "gbp_series_ranks", ranked=True)
    B, n_rows, V = x.shape
    ranker = lambda fold, p: _launch_ranks("gbp_series_ranks", (B, n_rows, V, x), B, n_rows, V, x.device, seg_start, seg_m, seg_n,      # noqa: E731
                                           fold, p, True, p.size > 0, False)
    return _rank_products(ranker, seg_start, seg_m, seg_n, max_lag, qs)


def _check_slots(ens, what):
    if torch.is_tensor(ens.k) and ens.k.ndim == 2 and ens.k.shape[1] > RANK_MAX_ROWS:
        raise ValueError("%s: at most %d slots per sounding (a padded column lives in LDS); the ensemble has %d" % (what, RANK_MAX_ROWS, ens.k.shape[1]))


def _ensemble_ranker(k, edges, sigma, ns, K, C, z, nd, start, seg_m, seg_n, s):
    """``ranker(fold, p, counts=True, values=False)`` of soundings ``s`` (a slice) through gbp_ensemble_ranks."""
    n = s.stop - s.start
    head = (n, ns, K, k[s], edges[s], sigma[s], nd, z)
    return lambda fold, p, counts=True, values=False: _launch_ranks("gbp_ensemble_ranks", head, n, ns, nd, k.device, start[s], seg_m[s], seg_n[s],
                                                                    fold, p, counts, p.size > 0, values)


def _rank_block(block, B, ns, nd):
    """Soundings per launch: ``block``, or as many as keep less, leq and the derived series beside them (32 B a sample) under 2 GiB."""
    return max(1, min(max(B, 1), RANK_BLOCK_BYTES // (32 * ns * nd))) if block is None else int(block)


def ensemble_ranks(ens, depth_edges, chains=1, fold=False, probabilities=None, counts=True, values=False):
    """``series_ranks`` of the series log10 conductivity at the centres of ``depth_edges`` [n_depth + 1] over the kept models, the
    series never read from memory (gbp_ensemble_ranks; the used samples are those of ``diagnostics``); one launch, [B, n_slots,
    n_depth] outputs.  ``values``: x_out, the values that were ranked."""
    p = check_probabilities(probabilities)
    _check_slots(ens, "ensemble_ranks")
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "ensemble_ranks", "gbp_ensemble_ranks", misfit=False)
    z = torch.as_tensor(z_np).to(k.device)
    out = _ensemble_ranker(k, edges, sigma, ns, K, C, z, int(z_np.size), start, seg_m, seg_n, slice(0, B))(fold, p, counts, values)
    out["n_chains_used"], out["segment_length"], out["n_segments"] = used, seg_n, seg_m
    return out


def rank_diagnostics(ens, depth_edges, chains=1, max_lag=None, percentiles=(5, 50, 95), block=None):
    """Did the chains run long enough for the percentiles?  Per sounding and cell of ``depth_edges`` [n_depth + 1], on the series
    and the used samples of ``diagnostics`` (``rank_diagnostics_reference`` states the rule): rhat_bulk, rhat_folded and rhat_rank =
    their maximum (rank-normalised split R-hat: free of the variable's scale, and the folded one sees chains that differ in spread),
    ess_bulk, tau_bulk, truncated_bulk, ess_percentile_<p> (the independent samples behind percentile p), ess_tail (the smaller of
    the lowest and the highest percentile's; NaN where the percentile sits on the sample's extreme) and quantile_<p>, the exact
    sample quantile, f64 [B, n_depth]; the same names with ``_k`` (the layer count) and ``_misfit`` (log10 of the misfit) [B];
    ess_bulk_min [B], the smallest finite ess_bulk over the cells (NaN: none); n_chains_used, segment_length, n_segments int32 [B].
    At most 16 384 slots.  ``block``: soundings per launch (None: as many as keep a block's counts and derived series under 2 GiB)."""
    max_lag = check_max_lag(max_lag)
    qs = check_percentiles(percentiles)
    _check_slots(ens, "rank_diagnostics")
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    check_block(block, "rank_diagnostics")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "rank_diagnostics", "gbp_ensemble_ranks", misfit=True)
    nd, dev = int(z_np.size), k.device
    z = torch.as_tensor(z_np).to(dev)
    step = _rank_block(block, B, ns, nd)
    parts = []
    for b0 in range(0, B, step):
        s = slice(b0, min(B, b0 + step))
        parts.append(_rank_products(_ensemble_ranker(k, edges, sigma, ns, K, C, z, nd, start, seg_m, seg_n, s), start[s], seg_m[s], seg_n[s], max_lag, qs))
    if not parts:
        parts.append(_rank_products(_ensemble_ranker(k, edges, sigma, ns, K, C, z, nd, start, seg_m, seg_n, slice(0, 0)), start, seg_m, seg_n, max_lag, qs))
    out = {name: torch.cat([q[name] for q in parts]) for name in parts[0]}
    scalars = torch.stack((k.to(torch.float64), torch.log10(ens.misfit.to(torch.float64))), dim=2).contiguous()
    ranker = lambda fold, p: _launch_ranks("gbp_series_ranks", (B, ns, 2, scalars), B, ns, 2, dev, start, seg_m, seg_n, fold, p, True,      # noqa: E731
                                           p.size > 0, False)
    two = _rank_products(ranker, start, seg_m, seg_n, max_lag, qs)
    for name in list(two):
        out[name + "_k"], out[name + "_misfit"] = two[name][:, 0], two[name][:, 1]
    out["n_chains_used"], out["segment_length"], out["n_segments"] = used, seg_n, seg_m
    ess = out["ess_bulk"]
    lowest = torch.where(torch.isfinite(ess), ess, torch.full_like(ess, float("inf"))).min(dim=1).values if nd else torch.full((B,), float("inf"), device=dev)
    out["ess_bulk_min"] = torch.where(torch.isfinite(lowest), lowest, torch.full_like(lowest, float("nan")))
    return out


def quantiles(ens, depth_edges, percentiles, chains=1, block=None):
    """The exact sample quantiles (numpy's ``method="linear"``) of log10 conductivity at the centres of ``depth_edges`` over the used
    kept models -- not the hit map's 250 value cells: {quantile_<p> f64 [B, n_depth], n_chains_used, segment_length, n_segments}.  One
    launch per block that writes no series (gbp_ensemble_ranks with no counts)."""
    qs = check_percentiles(percentiles)
    _check_slots(ens, "quantiles")
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    check_block(block, "quantiles")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "quantiles", "gbp_ensemble_ranks", misfit=False)
    nd, dev = int(z_np.size), k.device
    z = torch.as_tensor(z_np).to(dev)
    p = np.asarray([q / 100.0 for q in qs], dtype=np.float64)
    step = max(B, 1) if block is None else int(block)
    order = torch.cat([_ensemble_ranker(k, edges, sigma, ns, K, C, z, nd, start, seg_m, seg_n, slice(b0, min(B, b0 + step)))(False, p, False)["order"]
                       for b0 in range(0, max(B, 1), step)])
    nu = _used_count(seg_m, seg_n, order[:, 0, 0])
    out = {"quantile_" + percentile_name(q): sample_quantile(order, nu, i, p[i]) for i, q in enumerate(qs)}
    out["n_chains_used"], out["segment_length"], out["n_segments"] = used, seg_n, seg_m
    return out


# ---- weighted products ---------------------------------------------------------------------------------------------

WEIGHT_MAX_ROWS, WEIGHT_MAX_THRESHOLDS, WEIGHT_ONE = 4096, 8, 2 ** 40


def check_thresholds(thresholds):
    """``thresholds`` (None: none) as a float64 numpy list of at most 8 finite numbers."""
    if thresholds is None:
        return np.zeros(0, dtype=np.float64)
    t = np.asarray(thresholds, dtype=np.float64)
    if t.ndim != 1 or t.size > WEIGHT_MAX_THRESHOLDS:
        raise ValueError("thresholds: a list of at most %d numbers" % WEIGHT_MAX_THRESHOLDS)
    if not np.all(np.isfinite(t)):
        raise ValueError("thresholds: every one finite")
    return t


def quantise_weights(w, n_used):
    """The one step from floating-point weights to the integer multiplicities the weighted products take: ``w`` [B, n] (floating point;
    torch on any device, or numpy), ``n_used`` [B] integers in 0 .. n.  Per sounding, over the used rows u < n_used,
    q = rint(w / max_u w * 2^40): one IEEE division, one exact scaling, one rounding to the nearest integer (ties to even), so that
    torch on a device and numpy give the same integers.  Returns int64 [B, n] of the kind of ``w``: the largest weight maps to 2^40,
    the rows >= n_used to 0 whatever they hold.  A NaN, infinite or negative weight among the used rows is refused.  A sounding with
    n_used == 0 or all weights 0 gives q = 0.  A weight below 2^-41 of the largest becomes 0: twelve orders of magnitude below
    anything a Monte-Carlo sample of at most 4096 models can resolve."""
    tensor = torch.is_tensor(w)
    if not tensor:
        w = np.asarray(w)
    if w.ndim != 2 or not (w.dtype.is_floating_point if tensor else w.dtype.kind == "f"):
        raise ValueError("quantise_weights: w is floating point [B, n]")
    B, n = w.shape
    nu = n_used.detach().cpu().numpy() if torch.is_tensor(n_used) else np.asarray(n_used)
    if nu.shape != (B,) or nu.dtype.kind not in "iu" or (B and (nu.min() < 0 or nu.max() > n)):
        raise ValueError("quantise_weights: n_used holds one integer in 0 .. n per sounding")
    used = np.arange(n)[None, :] < nu[:, None]
    if tensor:
        used = torch.as_tensor(used).to(w.device)
        w = w.to(torch.float64)
        if bool((used & ~((w >= 0.0) & torch.isfinite(w))).any()):
            raise ValueError("quantise_weights: a NaN, infinite or negative weight among the used rows")
        if n == 0:
            return torch.zeros((B, 0), dtype=torch.int64, device=w.device)
        wu = torch.where(used, w, torch.zeros((), dtype=torch.float64, device=w.device))
        top = wu.max(dim=1, keepdim=True).values
        q = torch.round(wu / top * float(WEIGHT_ONE))
        return torch.where(used & (top > 0.0), q, torch.zeros_like(q)).to(torch.int64)
    w = w.astype(np.float64)
    if np.any(used & ~((w >= 0.0) & np.isfinite(w))):
        raise ValueError("quantise_weights: a NaN, infinite or negative weight among the used rows")
    if n == 0:
        return np.zeros((B, 0), dtype=np.int64)
    wu = np.where(used, w, 0.0)
    top = wu.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.rint(wu / top * float(WEIGHT_ONE))
    return np.where(used & (top > 0.0), q, 0.0).astype(np.int64)


def weighted_reference(x, rows, n_used, q, probabilities=None, thresholds=None, dtype=np.float64):
    """The rule of the weighted products in numpy: ``x`` [B, n_rows, V] (for an ensemble: log10 conductivity of the slots at the cell
    centres), ``rows`` integers [B, n], ``n_used`` [B], ``q`` int64 [B, n].  Model u < m = n_used[b] (clamped to 0 .. n) is row
    rows[b, u] with the INTEGER multiplicity q[b, u] (clamped to 0 .. 2^40; ``quantise_weights`` makes them from floating-point
    weights); a row with q == 0 takes no part whatever it holds or names, a participating row index is clamped into the rows.
    W = sum q; C(t) = sum of q over the participating values <= t (compared as doubles).  Returns

    ``total`` int64 [B] = W;
    ``quantile`` f64 [B, n_p, V]: the smallest participating value t with float64(C(t)) >= max(p * float64(W), 1.0) -- the inverse of
        the weighted ECDF, Hyndman & Fan's type 1; p = 0 gives the smallest value of positive weight.  With equal weights this is
        s[max(ceil(p n), 1) - 1] of the sorted column: NOT the interpolated ``quantiles`` (numpy's "linear", type 7);
    ``above`` int64 [B, n_t, V] = sum of q over the participating values >= the threshold (divided by W: the exceedance probability);
    ``mean`` = sum q x / W and ``sd`` = sqrt(sum q (x - mean)^2 / W) [B, V], two passes evaluated in ``dtype`` (np.longdouble: the
        yardstick of the rounding of the device's fp64 sums, whose order of addition is not part of the rule).

    W == 0: quantile, mean, sd NaN and above 0.  A column with a non-finite participating value: quantile, mean, sd NaN, above -1.
    Every decision is a comparison of integers (exact in fp64 up to 2^52 >= W): no order of addition or of ties can change a bit."""
    ft = np.dtype(dtype).type
    x, rows, q = np.asarray(x, dtype=np.float64), np.asarray(rows), np.asarray(q)
    nu = np.asarray(n_used).reshape(-1)
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("weighted_reference: x [B, n_rows, V]")
    B, n_rows, V = x.shape
    if rows.ndim != 2 or rows.shape[0] != B or not 1 <= rows.shape[1] <= WEIGHT_MAX_ROWS or rows.dtype.kind not in "iu":
        raise ValueError("weighted_reference: rows holds integers [B, n] with 1 <= n <= %d" % WEIGHT_MAX_ROWS)
    if q.shape != rows.shape or q.dtype.kind not in "iu" or nu.shape != (B,) or nu.dtype.kind not in "iu":
        raise ValueError("weighted_reference: q holds integers [B, n], n_used [B]")
    p, thr = check_probabilities(probabilities), check_thresholds(thresholds)
    n = rows.shape[1]
    total = np.zeros(B, dtype=np.int64)
    quantile, above = np.full((B, p.size, V), np.nan), np.zeros((B, thr.size, V), dtype=np.int64)
    mean, sd = np.full((B, V), np.nan, dtype=ft), np.full((B, V), np.nan, dtype=ft)
    for b in range(B):
        m = int(min(max(nu[b], 0), n))
        qq = np.clip(q[b, :m].astype(np.int64), 0, WEIGHT_ONE)
        W = int(qq.sum())
        total[b] = W
        if W == 0:
            continue
        part = qq > 0
        r, wq = np.clip(rows[b, :m][part].astype(np.int64), 0, n_rows - 1), qq[part]
        for v in range(V):
            c = x[b, r, v]
            if not np.all(np.isfinite(c)):
                above[b, :, v] = -1
                continue
            order = np.argsort(c, kind="stable")
            s = c[order]
            C = np.cumsum(wq[order])[np.searchsorted(s, s, side="right") - 1]      # C(s_i): ties share the weight of their run
            for i in range(p.size):
                quantile[b, i, v] = s[int(np.argmax(C.astype(np.float64) >= max(p[i] * np.float64(W), 1.0)))]
            for j in range(thr.size):
                above[b, j, v] = wq[c >= thr[j]].sum()
            cf, wf = c.astype(ft), wq.astype(ft)
            mean[b, v] = (wf * cf).sum() / ft(W)
            d = cf - mean[b, v]
            sd[b, v] = np.sqrt((wf * (d * d)).sum() / ft(W))
    return dict(total=total, quantile=quantile, above=above, mean=mean, sd=sd)


def _check_percentiles_or_none(percentiles):
    return () if percentiles is None or (np.ndim(percentiles) == 1 and np.size(percentiles) == 0) else check_percentiles(percentiles)


def _check_listed(rows, n_used, q, B, what, floating=False):
    """``rows`` int32 [B, n], ``n_used`` int32 [B], ``q`` int64 [B, n] (``floating``: or float64 weights) (torch, any device),
    1 <= n <= 4096."""
    if rows.ndim != 2 or rows.shape[0] != B or not 1 <= rows.shape[1] <= WEIGHT_MAX_ROWS:
        raise ValueError("%s: rows [B, n] with 1 <= n <= %d" % (what, WEIGHT_MAX_ROWS))
    if tuple(q.shape) != tuple(rows.shape) or tuple(n_used.shape) != (B,):
        raise ValueError("%s: q [B, n] as rows, n_used [B]" % what)
    if rows.dtype != torch.int32 or n_used.dtype != torch.int32 or not (q.dtype == torch.int64 or (floating and q.dtype == torch.float64)):
        raise TypeError("%s: rows and n_used are int32, q is int64" % what + (" (weights: float64 or int64)" if floating else ""))


def _launch_weighted(entry, head, B, V, dev, rows, n_used, q, p, thr):
    """One call of gbp_series_weighted / gbp_ensemble_weighted (``head``: the entry's arguments up to n) on fresh outputs."""
    out = dict(total=torch.empty(B, dtype=torch.int64, device=dev), quantile=torch.empty((B, p.size, V), dtype=torch.float64, device=dev),
               above=torch.empty((B, thr.size, V), dtype=torch.int64, device=dev))
    stats = torch.empty((B, 2, V), dtype=torch.float64, device=dev)
    given = lambda a: a if a.numel() else None      # noqa: E731
    if B > 0:
        _lib.call(entry, dev, *head, int(rows.shape[1]), rows, n_used, q, int(p.size), (ctypes.c_double * max(int(p.size), 1))(*p),
                  int(thr.size), (ctypes.c_double * max(int(thr.size), 1))(*thr), out["total"], given(out["quantile"]), given(out["above"]), stats)
    out["mean"], out["sd"] = stats[:, 0], stats[:, 1]
    return out


def series_weighted(x, rows, n_used, q, percentiles=(5, 50, 95), thresholds=()):
    """The weighted products (``weighted_reference`` states the rule) within the columns of the series ``x`` f64 [B, n_rows, V] on the
    device: ``rows`` int32 [B, n] (n <= 4096), ``n_used`` int32 [B], ``q`` int64 [B, n] integer multiplicities in 0 .. 2^40
    (``quantise_weights``).  Returns {total int64 [B], quantile f64 [B, n_p, V] at ``percentiles`` / 100 -- the type-1 inverse of the
    weighted ECDF, not the interpolated ``quantiles`` --, above int64 [B, n_t, V], mean, sd f64 [B, V]}.  One kernel
    (gbp_series_weighted)."""
    entry = "gbp_series_weighted"
    qs, thr = _check_percentiles_or_none(percentiles), check_thresholds(thresholds)
    are_tensors((x, rows, n_used, q), "ensembles", "series_weighted", entry)
    if x.dtype != torch.float64:
        raise TypeError("series_weighted: x is float64")
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("series_weighted: x is float64 [B, n_rows, V] with n_rows >= 1 and V >= 1")
    _check_listed(rows, n_used, q, x.shape[0], "series_weighted")
    on_device((x, rows, n_used, q), "ensembles", "series_weighted", entry)
    B, n_rows, V = x.shape
    p = np.asarray([v / 100.0 for v in qs], dtype=np.float64)
    return _launch_weighted(entry, (B, n_rows, V, x.contiguous()), B, V, x.device, rows.contiguous(), n_used.contiguous(), q.contiguous(), p, thr)


def weighted(ens, depth_edges, rows, weight, n_used=None, percentiles=(5, 50, 95), thresholds=(), block=None):
    """The posterior of every sounding under weights on its kept models: per sounding and cell of ``depth_edges`` [n_depth + 1] the
    weighted mean, sd, percentiles and exceedance probabilities of log10 conductivity at the cell centre (``weighted_reference``
    states the rule), the series never read from memory (gbp_ensemble_weighted).  ``rows`` int32 [B, n] (n <= 4096): model u of
    sounding b is slot rows[b, u]; ``n_used`` int32 [B] (None: all n); ``weight`` [B, n]: float64 -- the smoothed marginals of
    ``sections.sections``, a borehole's likelihood, importance weights: quantised by ``quantise_weights`` -- or int64, taken as the
    multiplicities themselves (dwell counts).  ``thresholds``: at most 8, in log10 S/m.

    Returns on the device ``mean``, ``sd``, ``percentile_<p>`` (``percentile_name``) f64 [B, n_depth]; ``exceedance`` f64 [B, n_t,
    n_depth], the weight of the models >= the threshold over the total (NaN where the total is 0 or the column holds a non-finite
    value); ``weight_total`` int64 [B], the sum W of the multiplicities; ``n_effective`` f64 [B] = W^2 / sum q^2 (NaN: W == 0).
    The percentiles are the type-1 inverse of the weighted ECDF -- a value one of the models holds --, NOT the interpolated
    ``quantiles``.  ``block``: soundings per launch (None: as many as keep a launch under 2^32 - 1 threads)."""
    entry = "gbp_ensemble_weighted"
    qs, thr = check_percentiles(percentiles), check_thresholds(thresholds)
    z_np = centres(depth_edges)
    check_block(block, "weighted")
    tensors = (ens.k, ens.edges, ens.sigma, rows, weight) + (() if n_used is None else (n_used,))
    are_tensors(tensors, "ensembles", "weighted", entry)
    k, edges, sigma, B, ns, K = check_ensemble(ens)
    if ns < 1 or not 1 <= K <= 64:
        raise ValueError("ensemble: at least one slot and K in [1, 64]")
    if weight.dtype not in (torch.float64, torch.int64):
        raise TypeError("weighted: weight is float64 (quantised) or int64 (the multiplicities)")
    if n_used is None:
        n_used = torch.full((B,), rows.shape[1] if rows.ndim == 2 else 0, dtype=torch.int32, device=rows.device)
    _check_listed(rows, n_used, weight, B, "weighted", floating=True)
    q = weight if weight.dtype == torch.int64 else quantise_weights(weight, n_used.clamp(min=0, max=rows.shape[1]))
    on_device(tensors, "ensembles", "weighted", entry)
    nd, dev, n = int(z_np.size), k.device, rows.shape[1]
    rows, n_used, q = rows.contiguous(), n_used.contiguous(), q.contiguous()
    z = torch.as_tensor(z_np).to(dev)
    p = np.asarray([v / 100.0 for v in qs], dtype=np.float64)
    P = 1 << max(n - 1, 0).bit_length()
    tiles = -(-nd // min(64, 8192 // P))
    step = max(1, (2 ** 32 - 1) // (1024 * tiles)) if block is None else int(block)
    parts = [_launch_weighted(entry, (s.stop - s.start, ns, K, k[s], edges[s], sigma[s], nd, z), s.stop - s.start, nd, dev, rows[s], n_used[s], q[s], p, thr)
             for s in (slice(b0, min(B, b0 + step)) for b0 in range(0, max(B, 1), step))]
    r = {name: torch.cat([part[name] for part in parts]) for name in parts[0]}
    out = dict(mean=r["mean"], sd=r["sd"])
    for i, v in enumerate(qs):
        out["percentile_" + percentile_name(v)] = r["quantile"][:, i]
    W = r["total"].to(torch.float64)
    nanv = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    out["exceedance"] = torch.where(r["above"] >= 0, r["above"].to(torch.float64) / W[:, None, None], nanv)
    out["weight_total"] = r["total"]
    live = torch.arange(n, device=dev)[None, :] < n_used[:, None]
    qf = torch.where(live, q.clamp(min=0, max=WEIGHT_ONE), torch.zeros_like(q)).to(torch.float64)
    out["n_effective"] = W * W / (qf * qf).sum(dim=1)
    return out


def correlation_reference(x, seg_start, n, band, dtype=np.float64, normalise=True):
    """The rule of the correlation between variables for one sounding, in numpy: ``x`` [n_rows, V], M = len(seg_start) segments of
    ``n`` rows each (the lists ``segments`` builds: the used samples are the ones the diagnostics use), evaluated in ``dtype``.
    Returns {mean, sd [V], band [V, W + 1]} with W = ``band`` (0 .. V - 1).

    With n_used = M n used rows: mu_v = (1/n_used) sum_t x_tv, d = x - mu, C(u, v) = (1/(n_used - 1)) sum_t d_tu d_tv (the pooled sample
    covariance), sd_v = sqrt(C(v, v)), R(u, v) = C(u, v) / (sd_u sd_v); band[c, j] = R(c, c + j) (``normalise=False``: C(c, c + j)), NaN
    where c + j >= V.  M == 0 or n_used < 4: everything NaN.  A variable whose used samples are all one value (compared as stored):
    mean = it, sd = 0, every band entry that involves it NaN, its own diagonal included; one with a non-finite used sample: mean, sd
    and its entries NaN; no other entry is touched by either.  R of a live variable with itself is 1 exactly.

    ``sd`` is the POOLED sample standard deviation (one mean for all segments, divisor n_used - 1); the diagnostics' sd = sqrt(vp)
    (within-segment variance (n - 1)/n W plus the variance of the segment means) differs from it by O(1/n) for segments whose means
    agree to O(sd / sqrt(n)): the spread of the segment means enters the two with weights 1/M and 1/(M - 1)."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("correlation_reference: x [n_rows, V]")
    V = x.shape[1]
    if isinstance(band, bool) or int(band) != band or not 0 <= int(band) <= V - 1:
        raise ValueError("correlation_reference: band must be an integer in 0 .. V - 1")
    W = int(band)
    starts = [int(q) for q in np.asarray(seg_start).reshape(-1)]
    M, N = len(starts), int(n)
    if M > MAX_SEGMENTS:
        raise ValueError("correlation_reference: at most %d segments" % MAX_SEGMENTS)
    out = dict(mean=np.full(V, np.nan, dtype=dtype), sd=np.full(V, np.nan, dtype=dtype), band=np.full((V, W + 1), np.nan, dtype=dtype))
    if M == 0 or M * N < 4:
        return out
    if min(starts) < 0 or max(starts) + N > x.shape[0]:
        raise ValueError("correlation_reference: a segment leaves the rows 0 .. %d" % (x.shape[0] - 1))
    stored = np.concatenate([x[q:q + N] for q in starts])               # [n_used, V]
    xs = stored.astype(dtype)
    nu = dtype(M * N)
    bad = ~np.all(np.isfinite(stored), axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        const = ~bad & (stored.min(axis=0) == stored.max(axis=0))
        dead = bad | const
        mu = xs.sum(axis=0) / nu
        d = np.where(dead[None, :], dtype(0), xs - mu[None, :])
        var = (d * d).sum(axis=0) / (nu - dtype(1))
        sd = np.sqrt(var)
        for j in range(W + 1):
            c = (d[:, :V - j] * d[:, j:]).sum(axis=0) / (nu - dtype(1))
            if normalise:
                c = c / (sd[:V - j] * sd[j:]) if j else np.ones(V, dtype=dtype)
            c[dead[:V - j] | dead[j:]] = np.nan
            out["band"][:V - j, j] = c
    mu[const] = stored[0, const].astype(dtype)
    mu[bad] = np.nan
    sd[const] = 0
    sd[bad] = np.nan
    out["mean"], out["sd"] = mu, sd
    return out


def band_to_matrix(band):
    """The symmetric matrix [..., V, V] of a band [..., V, W + 1] (band[..., c, j] = entry (c, c + j)); NaN outside the band.  Torch or
    numpy, as given."""
    if band.ndim < 2 or not 1 <= band.shape[-1] <= band.shape[-2]:
        raise ValueError("band_to_matrix: band [..., V, W + 1] with 0 <= W <= V - 1")
    V, W1 = band.shape[-2], band.shape[-1]
    if torch.is_tensor(band):
        out = torch.full(tuple(band.shape[:-1]) + (V,), float("nan"), dtype=band.dtype, device=band.device)
    else:
        out = np.full(band.shape[:-1] + (V,), np.nan, dtype=band.dtype)
    for j in range(W1):
        c = np.arange(V - j)
        out[..., c, c + j] = band[..., :V - j, j]
        out[..., c + j, c] = band[..., :V - j, j]
    return out


def check_threshold(threshold):
    """``threshold`` as a float strictly between 0 and 1."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0.0 < float(threshold) < 1.0:
        raise ValueError("threshold must be a number with 0 < threshold < 1")
    return float(threshold)


def correlation_runs_reference(band, threshold):
    """The runs of a band [V, W + 1] above ``threshold``, in numpy: for cell c, ``down[c]`` = the number of consecutive j = 1, 2, ...
    with j <= W, c + j <= V - 1 and band[c, j] >= threshold (NaN compares false and ends the run), ``up[c]`` the same with
    band[c - j, j] and c - j >= 0; ``closed_down[c]`` / ``closed_up[c]``: the walk ended at an entry that is not >= threshold (False:
    it ended at j = W or at the end of the axis, so the run is a lower bound).  A cell whose diagonal is NaN: up = down = 0, both
    flags False.  Returns {up, down int32 [V], closed_up, closed_down bool [V]}."""
    band = np.asarray(band)
    if band.ndim != 2 or not 1 <= band.shape[1] <= band.shape[0]:
        raise ValueError("correlation_runs_reference: band [V, W + 1] with 0 <= W <= V - 1")
    V, W = band.shape[0], band.shape[1] - 1
    up, down = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    cu, cd = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    for c in range(V):
        if np.isnan(band[c, 0]):
            continue
        j = 1
        while j <= W and c + j <= V - 1:
            if not band[c, j] >= threshold:
                cd[c] = True
                break
            down[c] += 1
            j += 1
        j = 1
        while j <= W and c - j >= 0:
            if not band[c - j, j] >= threshold:
                cu[c] = True
                break
            up[c] += 1
            j += 1
    return dict(up=up, down=down, closed_up=cu, closed_down=cd)


def resolution_length(up, down, depth_edges, live=None):
    """edges[c + down + 1] - edges[c - up] in metres: the thickness of the run of cells that move with cell c (at least the cell's own
    thickness).  ``up`` / ``down`` int [..., V] (torch or numpy), ``depth_edges`` [V + 1]; ``live`` bool [..., V] (None: everything):
    NaN where it is False (the cells whose diagonal is NaN)."""
    centres(depth_edges)
    e = np.asarray(depth_edges, dtype=np.float64).reshape(-1)
    V = e.size - 1
    if up.shape != down.shape or up.shape[-1] != V:
        raise ValueError("resolution_length: up and down [..., V] for depth_edges [V + 1]")
    if torch.is_tensor(up):
        c = torch.arange(V, device=up.device)
        et = torch.as_tensor(e).to(up.device)
        out = et[(c + down.long() + 1).clamp(max=V)] - et[(c - up.long()).clamp(min=0)]
        return out if live is None else torch.where(live, out, torch.full_like(out, float("nan")))
    c = np.arange(V)
    out = e[np.minimum(c + np.asarray(down, dtype=np.int64) + 1, V)] - e[np.maximum(c - np.asarray(up, dtype=np.int64), 0)]
    return out if live is None else np.where(live, out, np.nan)


def check_band(band, V):
    """``band`` (None: V - 1) as an int >= 0, clipped to V - 1."""
    if band is None:
        return V - 1
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or int(band) < 0:
        raise ValueError("band must be an integer >= 0")
    return min(int(band), V - 1)


def series_correlation(x, seg_start, seg_m, seg_n, band=None, normalise=True, rank=False):
    """The correlation between the variables (``correlation_reference`` states the rule) of the series ``x`` f64 [B, n_rows, V] on the
    device, segments as ``series_diagnostics`` takes them.  Returns {mean, sd f64 [B, V], band f64 [B, V, W + 1]}: band[b, c, j] =
    R(c, c + j) (``normalise=False``: the covariance), W = ``band`` clipped to V - 1 (None: V - 1, the whole matrix;
    ``band_to_matrix`` unfolds it).  gbp_series_correlation: centred products on the fp64 matrix cores.  ``rank``: Spearman's -- the
    same on the midranks of every column (``series_ranks``: n_rows <= 16 384, disjoint segments); mean and sd are the midranks'."""
    x, seg_start, seg_m, seg_n, W = _check_series(x, seg_start, seg_m, seg_n, "series_correlation", "gbp_series_correlation",
                                                  check_v=lambda V: check_band(band, V), ranked=bool(rank))
    if rank:
        r = series_ranks(x, seg_start, seg_m, seg_n)
        x = midranks(r["less"], r["leq"])
    (B, n_rows, V), dev = x.shape, x.device
    stats = torch.empty((B, 2, V), dtype=torch.float64, device=dev)
    out = torch.empty((B, V, W + 1), dtype=torch.float64, device=dev)
    if B > 0:
        _lib.call("gbp_series_correlation", dev, B, n_rows, V, x, int(seg_start.shape[1]), seg_start, seg_m, seg_n, W, int(bool(normalise)), stats, out)
    return dict(mean=stats[:, 0], sd=stats[:, 1], band=out)


def correlation_runs(band, threshold):
    """``correlation_runs_reference`` on a device band f64 [B, V, W + 1] (gbp_band_runs): {up, down int32 [B, V], closed_up,
    closed_down bool [B, V]}.  ``threshold``: any number that is not NaN."""
    are_tensors((band,), "ensembles", "correlation_runs", "gbp_band_runs")
    if band.dtype != torch.float64:
        raise TypeError("correlation_runs: band is float64")
    if band.ndim != 3 or not 1 <= band.shape[2] <= band.shape[1]:
        raise ValueError("correlation_runs: band [B, V, W + 1] with 0 <= W <= V - 1")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("correlation_runs: threshold is NaN")
    on_device((band,), "ensembles", "correlation_runs", "gbp_band_runs")
    band, dev = band.contiguous(), band.device
    B, V, W1 = band.shape
    up, down = (torch.empty((B, V), dtype=torch.int32, device=dev) for _ in range(2))
    closed = torch.empty((B, 2, V), dtype=torch.uint8, device=dev)
    if B > 0:
        _lib.call("gbp_band_runs", dev, B, V, W1 - 1, band, threshold, up, down, closed)
    return dict(up=up, down=down, closed_up=closed[:, 0].bool(), closed_down=closed[:, 1].bool())


BAND_BLOCK_BYTES = 2 << 30


def correlation(ens, depth_edges, chains=1, band=64, threshold=0.5, normalise=True, block=None, keep_band=True, rank=False):
    """What moves together, and over what thickness?  Per sounding the posterior correlation between the cells of ``depth_edges``
    [n_depth + 1] of the series log10 conductivity at the cell centre over the kept models (``correlation_reference`` states the rule;
    the used samples are those of ``diagnostics``: ``segments``, ``chains`` = C as there), the series never written to memory
    (gbp_ensemble_correlation).  Returns mean, sd f64 [B, n_depth] (sd: the pooled sample standard deviation, O(1/N) from the
    diagnostics' sd); ``band`` f64 [B, n_depth, W + 1], band[b, c, j] = R(c, c + j), W = ``band`` clipped to n_depth - 1
    (``normalise=False``: covariances; dropped with ``keep_band=False``); the runs of entries >= ``threshold`` (0 < threshold < 1) up
    and down from every cell (``correlation_runs_reference``): up, down int32, closed_up, closed_down bool [B, n_depth];
    resolution_cells = up + down + 1; resolution_length f64 [B, n_depth] (``resolution_length``: metres, NaN for a cell that is
    constant or non-finite) and resolution_closed = closed_up & closed_down (False: the length is a lower bound -- the run reached
    the band's width or the end of the axis); n_chains_used, segment_length, n_segments int32 [B].  ``block``: soundings per launch
    (None: as many as keep a block's band under 2 GiB).  ``rank``: Spearman's correlation -- per block the midranks of every column
    (gbp_ensemble_ranks) are written as a series [block, n_slots, n_depth] and correlated through gbp_series_correlation; mean and
    sd are then the midranks'; at most 16 384 slots, and None for ``block`` keeps that series under 2 GiB too."""
    if rank:
        _check_slots(ens, "correlation(rank=True)")
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    nd = int(z_np.size)
    W = check_band(band, nd)
    threshold = check_threshold(threshold)
    check_block(block, "correlation")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "correlation", "gbp_ensemble_correlation", misfit=False)
    dev = k.device
    step = max(1, BAND_BLOCK_BYTES // (nd * (W + 1) * 8)) if block is None else int(block)
    if rank and block is None:
        step = min(step, _rank_block(None, B, ns, nd))
    stats = torch.empty((B, 2, nd), dtype=torch.float64, device=dev)
    full = torch.empty((B, nd, W + 1), dtype=torch.float64, device=dev) if keep_band else None
    up, down = (torch.empty((B, nd), dtype=torch.int32, device=dev) for _ in range(2))
    closed = torch.empty((B, 2, nd), dtype=torch.uint8, device=dev)
    live = torch.empty((B, nd), dtype=torch.bool, device=dev)
    if B > 0:
        z = torch.as_tensor(z_np).to(dev)
        work = None if keep_band else torch.empty((min(step, B), nd, W + 1), dtype=torch.float64, device=dev)
        for b0 in range(0, B, step):
            s = slice(b0, min(B, b0 + step))
            part = full[s] if keep_band else work[:s.stop - s.start]
            if rank:
                r = _ensemble_ranker(k, edges, sigma, ns, K, C, z, nd, start, seg_m, seg_n, s)(False, np.zeros(0))
                mid = midranks(r["less"], r["leq"])
                del r
                _lib.call("gbp_series_correlation", dev, s.stop - s.start, ns, nd, mid, 2 * C, start[s], seg_m[s], seg_n[s], W, int(bool(normalise)),
                          stats[s], part)
                del mid
            else:
                _lib.call("gbp_ensemble_correlation", dev, s.stop - s.start, ns, K, k[s], edges[s], sigma[s], nd, z, 2 * C, start[s], seg_m[s], seg_n[s],
                          W, int(bool(normalise)), stats[s], part)
            _lib.call("gbp_band_runs", dev, s.stop - s.start, nd, W, part, threshold, up[s], down[s], closed[s])
            live[s] = ~torch.isnan(part[:, :, 0])
    out = dict(mean=stats[:, 0], sd=stats[:, 1], up=up, down=down, closed_up=closed[:, 0].bool(), closed_down=closed[:, 1].bool())
    if keep_band:
        out["band"] = full
    out["resolution_cells"] = up + down + 1
    out["resolution_length"] = resolution_length(up, down, depth_edges, live=live)
    out["resolution_closed"] = out["closed_up"] & out["closed_down"]
    out["n_chains_used"], out["segment_length"], out["n_segments"] = used, seg_n, seg_m
    return out


def save(ens, path):
    """Write an ``Ensemble`` to ``path`` with np.savez_compressed; returns the path."""
    np.savez_compressed(path, **{n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in ens._asdict().items()})
    return path


def load(path, device=None):
    """The ``Ensemble`` ``save`` wrote, as numpy arrays -- or as torch tensors on ``device`` (what ``realisations`` / ``rebin`` take)."""
    with np.load(path) as f:
        d = {n: f[n] for n in Ensemble._fields}
    d["thin"] = int(d["thin"])
    if device is not None:
        d = {n: (torch.as_tensor(v).to(device) if n != "thin" else v) for n, v in d.items()}
    return Ensemble(**d)


def _parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m geobipy_amd.ensembles",
                                description="Chain diagnostics (ESS, autocorrelation time, split R-hat) of a saved ensemble; writes <name>.diagnostics.npz")
    p.add_argument("ensemble", help="an ensemble written by ensembles.save (.npz)")
    axis = p.add_mutually_exclusive_group(required=True)
    axis.add_argument("--depth-edges", type=float, nargs="+", metavar="EDGE", help="ascending cell edges [n_depth + 1]")
    axis.add_argument("--depth-axis", nargs=2, metavar=("N", "WIDTH"), help="N uniform cells of WIDTH starting at 0")
    p.add_argument("--chains", type=int, default=1, help="replicate chains on the slot axis (default 1)")
    p.add_argument("--max-lag", type=int, default=None, help="largest lag, 1 .. 255 (default 255)")
    p.add_argument("--correlation", type=int, nargs="?", const=64, default=None, metavar="BAND",
                   help="instead of the diagnostics: the correlation between depth cells up to BAND cells apart (default 64) and the "
                        "resolution length; writes <name>.correlation.npz")
    p.add_argument("--threshold", type=float, default=None, metavar="T", help="with --correlation: cells move together while R >= T, 0 < T < 1 (default 0.5)")
    p.add_argument("--spearman", action="store_true", help="with --correlation: correlate the midranks of the columns (Spearman's correlation)")
    p.add_argument("--rank", action="store_true",
                   help="instead of the diagnostics: the rank diagnostics (rank-normalised and folded split R-hat, bulk and tail ESS, the ESS "
                        "behind every percentile, exact sample quantiles); writes <name>.rank_diagnostics.npz")
    p.add_argument("--percentiles", type=float, nargs="+", default=None, metavar="P", help="with --rank: ascending percentiles in [0, 100] (default 5 50 95)")
    p.add_argument("--device", default="cuda:0")
    return p


def parse_args(argv=None):
    """The command line of ``python -m geobipy_amd.ensembles`` as (path, depth_edges, chains, max_lag, device); refuses before any device work."""
    p = _parser()
    a = p.parse_args(argv)
    if a.depth_axis is not None:
        try:
            n, w = int(a.depth_axis[0]), float(a.depth_axis[1])
        except ValueError:
            p.error("--depth-axis N WIDTH: an integer and a number")
        if n < 1 or not (np.isfinite(w) and w > 0.0):
            p.error("--depth-axis: N >= 1 and a finite, positive WIDTH")
        edges = np.arange(n + 1, dtype=np.float64) * w
    else:
        edges = np.asarray(a.depth_edges, dtype=np.float64)
    try:
        centres(edges)
        max_lag = check_max_lag(a.max_lag)
        if not 1 <= a.chains <= MAX_SEGMENTS // 2:
            raise ValueError("--chains must be in 1 .. %d" % (MAX_SEGMENTS // 2))
    except ValueError as e:
        p.error(str(e))
    return a.ensemble, edges, a.chains, max_lag, a.device


def diagnostics_path(path):
    """<name>.diagnostics.npz beside the ensemble <name>.npz."""
    return (path[:-4] if path.endswith(".npz") else path) + ".diagnostics.npz"


def parse_correlation(argv=None):
    """``--correlation [BAND] [--threshold T]`` of the command line as (band, threshold), or None without ``--correlation``; refuses
    before any device work."""
    p = _parser()
    a = p.parse_args(argv)
    if a.correlation is None:
        if a.threshold is not None:
            p.error("--threshold needs --correlation")
        return None
    if a.correlation < 0:
        p.error("--correlation: BAND >= 0")
    if a.max_lag is not None:
        p.error("--max-lag belongs to the diagnostics (drop --correlation)")
    try:
        return a.correlation, check_threshold(0.5 if a.threshold is None else a.threshold)
    except ValueError as e:
        p.error("--threshold: " + str(e))


def correlation_path(path):
    """<name>.correlation.npz beside the ensemble <name>.npz."""
    return (path[:-4] if path.endswith(".npz") else path) + ".correlation.npz"


def parse_rank(argv=None):
    """``--rank [--percentiles P ...]`` and ``--spearman`` of the command line as (percentiles or None without ``--rank``, spearman);
    refuses before any device work."""
    p = _parser()
    a = p.parse_args(argv)
    if a.spearman and a.correlation is None:
        p.error("--spearman needs --correlation")
    if not a.rank:
        if a.percentiles is not None:
            p.error("--percentiles needs --rank")
        return None, a.spearman
    if a.correlation is not None:
        p.error("--rank and --correlation are two runs")
    try:
        return check_percentiles((5, 50, 95) if a.percentiles is None else a.percentiles), False
    except ValueError as e:
        p.error("--" + str(e))


def rank_diagnostics_path(path):
    """<name>.rank_diagnostics.npz beside the ensemble <name>.npz."""
    return (path[:-4] if path.endswith(".npz") else path) + ".rank_diagnostics.npz"


def main(argv=None):
    path, edges, chains, max_lag, device = parse_args(argv)
    corr = parse_correlation(argv)
    percentiles, spearman = parse_rank(argv)
    if percentiles is not None:
        ens = load(path, device=device)
        d = rank_diagnostics(ens, edges, chains=chains, max_lag=max_lag, percentiles=percentiles)
        out = rank_diagnostics_path(path)
        np.savez_compressed(out, depth_edges=edges, thin=ens.thin, percentiles=np.asarray(percentiles), **{n: v.cpu().numpy() for n, v in d.items()})
        print("wrote", out)
        return out
    if corr is not None:
        ens = load(path, device=device)
        d = correlation(ens, edges, chains=chains, band=corr[0], threshold=corr[1], rank=spearman)
        out = correlation_path(path)
        np.savez_compressed(out, depth_edges=edges, thin=ens.thin, threshold=corr[1], **{n: v.cpu().numpy() for n, v in d.items()})
        print("wrote", out)
        return out
    ens = load(path, device=device)
    d = diagnostics(ens, edges, chains=chains, max_lag=max_lag)
    out = diagnostics_path(path)
    np.savez_compressed(out, depth_edges=edges, thin=ens.thin, **{n: v.cpu().numpy() for n, v in d.items()})
    print("wrote", out)
    return out


if __name__ == "__main__":
    main()
