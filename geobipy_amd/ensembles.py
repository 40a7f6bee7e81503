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

There is no host fallback: all refuse tensors that are not on the device (``realisations_reference`` states the raster's rule in numpy,
``diagnostics_reference`` that of the diagnostics, ``correlation_reference`` and ``correlation_runs_reference`` those of the correlation).
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib

Ensemble = namedtuple("Ensemble", ("k", "edges", "sigma", "misfit", "count", "thin", "log_mean_prior"))
Ensemble.__doc__ = """k int32 [B, n_keep] (0: empty slot), edges / sigma f64 [B, n_keep, K] (a slot's k - 1 interface depths then +inf,
its k conductivities then NaN), misfit f64 [B, n_keep] (chi^2), count [B] (filled slots: they are the first ``count`` ones of a
single chain), thin (every thin-th accumulated sample was kept), log_mean_prior f64 [B] (ln of the chain's prior mean conductivity)."""


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


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
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    for a in (k, edges, sigma):
        if not torch.is_tensor(a) or a.device.type != "cuda":
            raise _lib.NativeLibraryError("ensembles.%s runs on the device (gbp_ensemble_%s); there is no host fallback" % (what[0], what[1]))
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or tuple(edges.shape[:2]) != tuple(k.shape):
        raise ValueError("ensemble: k [B, n_keep], edges and sigma [B, n_keep, K]")
    if k.dtype != torch.int32 or edges.dtype != torch.float64 or sigma.dtype != torch.float64:
        raise TypeError("ensemble: k is int32, edges and sigma are float64")
    B, ne, K = edges.shape
    if not 1 <= ne <= 4096 or not 1 <= K <= 64:
        raise ValueError("ensemble: n_keep must be in [1, 4096] and K in [1, 64]")
    return k.contiguous(), edges.contiguous(), sigma.contiguous(), B, ne, K


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
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gbp_ensemble_raster(B, ne, K, k.data_ptr(), edges.data_ptr(), sigma.data_ptr(), int(s_np.size), s.data_ptr(),
                                                       int(z_np.size), z.data_ptr(), out.data_ptr(), _stream(dev)))
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
    ptr = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gbp_ensemble_rebin(B, ne, K, k.data_ptr(), edges.data_ptr(), sigma.data_ptr(), lmp.data_ptr(), nv, hw, nd, width,
                                                      ptr(hm), M, bits, ptr(uz), ptr(uh), T, (ctypes.c_double * 4)(*(list(th) + [1.0] * (4 - T))),
                                                      (ctypes.c_int32 * 4)(*([int(d) for d in di] + [1] * (4 - T))), ptr(fh), ptr(fn), _stream(dev)))
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


def _on_device(tensors, what, entry):
    """The last check of an entry: shapes, dtypes and values are refused first, whatever device the tensors are on."""
    for a in tensors:
        if a.device.type != "cuda":
            raise _lib.NativeLibraryError("ensembles.%s runs on the device (%s); there is no host fallback" % (what, entry))


def _are_tensors(tensors, what, entry):
    for a in tensors:
        if not torch.is_tensor(a):
            raise _lib.NativeLibraryError("ensembles.%s takes torch tensors on the device (%s); there is no host fallback" % (what, entry))


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


def _check_series(x, seg_start, seg_m, seg_n, what, entry, check_v=lambda V: None):
    """The checks ``series_diagnostics`` and ``series_correlation`` share, in their order: tensors, x, ``check_v(V)`` (the entry's own
    check that needs V), the segment lists, and the device last.  Returns x and the lists, contiguous, and what ``check_v`` gave."""
    _are_tensors((x, seg_start, seg_m, seg_n), what, entry)
    if x.dtype != torch.float64:
        raise TypeError("%s: x is float64" % what)
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[1] > 32768:
        raise ValueError("%s: x is float64 [B, n_rows, V] with 1 <= n_rows <= 32768 and V >= 1" % what)
    own = check_v(x.shape[2])
    seg_start, seg_m, seg_n = _check_segments(seg_start, seg_m, seg_n, x.shape[0], x.shape[1], what)
    _on_device((x, seg_start, seg_m, seg_n), what, entry)
    return x.contiguous(), seg_start, seg_m, seg_n, own


def _check_block(block, what):
    if block is not None and (isinstance(block, bool) or int(block) != block or int(block) < 1):
        raise ValueError("%s: block must be a positive integer" % what)


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
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gbp_series_diagnostics(B, n_rows, V, x.data_ptr(), int(seg_start.shape[1]), seg_start.data_ptr(), seg_m.data_ptr(),
                                                          seg_n.data_ptr(), max_lag, stats.data_ptr(), pairs.data_ptr(),
                                                          None if rho is None else rho.data_ptr(), _stream(dev)))
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
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    tensors = (k, edges, sigma, ens.misfit) if misfit else (k, edges, sigma)
    _are_tensors(tensors, what, entry)
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or tuple(edges.shape[:2]) != tuple(k.shape) or (misfit and ens.misfit.shape != k.shape):
        raise ValueError("ensemble: %s [B, n_slots], edges and sigma [B, n_slots, K]" % ("k and misfit" if misfit else "k"))
    if k.dtype != torch.int32 or edges.dtype != torch.float64 or sigma.dtype != torch.float64 or (misfit and not ens.misfit.dtype.is_floating_point):
        raise TypeError("ensemble: k is int32, edges and sigma are float64" + (", misfit is floating point" if misfit else ""))
    B, ns, K = edges.shape
    C = check_chains(chains, ns)
    if not 1 <= ns <= 4096 * C or not 1 <= K <= 64:
        raise ValueError("ensemble: at most 4096 slots per chain and K in [1, 64]")
    _on_device(tensors, what, entry)
    k, edges, sigma, dev = k.contiguous(), edges.contiguous(), sigma.contiguous(), k.device
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
    _check_block(block, "diagnostics")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "diagnostics", "gbp_ensemble_diagnostics", misfit=True)
    nd, dev = int(z_np.size), k.device
    stats = torch.empty((B, 6, nd), dtype=torch.float64, device=dev)
    pairs = torch.empty((B, nd), dtype=torch.int32, device=dev)
    rho = torch.empty((B, max_lag + 1, nd), dtype=torch.float64, device=dev) if return_rho else None
    if B > 0:
        z = torch.as_tensor(z_np).to(dev)
        step = B if block is None else int(block)
        lib = _lib.load()
        with torch.cuda.device(dev):
            for b0 in range(0, B, step):
                s = slice(b0, min(B, b0 + step))
                _lib.check(lib.gbp_ensemble_diagnostics(s.stop - s.start, ns, K, k[s].data_ptr(), edges[s].data_ptr(), sigma[s].data_ptr(), nd,
                                                        z.data_ptr(), 2 * C, start[s].data_ptr(), seg_m[s].data_ptr(), seg_n[s].data_ptr(), max_lag,
                                                        stats[s].data_ptr(), pairs[s].data_ptr(), None if rho is None else rho[s].data_ptr(),
                                                        _stream(dev)))
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


def series_correlation(x, seg_start, seg_m, seg_n, band=None, normalise=True):
    """The correlation between the variables (``correlation_reference`` states the rule) of the series ``x`` f64 [B, n_rows, V] on the
    device, segments as ``series_diagnostics`` takes them.  Returns {mean, sd f64 [B, V], band f64 [B, V, W + 1]}: band[b, c, j] =
    R(c, c + j) (``normalise=False``: the covariance), W = ``band`` clipped to V - 1 (None: V - 1, the whole matrix;
    ``band_to_matrix`` unfolds it).  gbp_series_correlation: centred products on the fp64 matrix cores."""
    x, seg_start, seg_m, seg_n, W = _check_series(x, seg_start, seg_m, seg_n, "series_correlation", "gbp_series_correlation",
                                                  check_v=lambda V: check_band(band, V))
    (B, n_rows, V), dev = x.shape, x.device
    stats = torch.empty((B, 2, V), dtype=torch.float64, device=dev)
    out = torch.empty((B, V, W + 1), dtype=torch.float64, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gbp_series_correlation(B, n_rows, V, x.data_ptr(), int(seg_start.shape[1]), seg_start.data_ptr(), seg_m.data_ptr(),
                                                          seg_n.data_ptr(), W, int(bool(normalise)), stats.data_ptr(), out.data_ptr(), _stream(dev)))
    return dict(mean=stats[:, 0], sd=stats[:, 1], band=out)


def correlation_runs(band, threshold):
    """``correlation_runs_reference`` on a device band f64 [B, V, W + 1] (gbp_band_runs): {up, down int32 [B, V], closed_up,
    closed_down bool [B, V]}.  ``threshold``: any number that is not NaN."""
    _are_tensors((band,), "correlation_runs", "gbp_band_runs")
    if band.dtype != torch.float64:
        raise TypeError("correlation_runs: band is float64")
    if band.ndim != 3 or not 1 <= band.shape[2] <= band.shape[1]:
        raise ValueError("correlation_runs: band [B, V, W + 1] with 0 <= W <= V - 1")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("correlation_runs: threshold is NaN")
    _on_device((band,), "correlation_runs", "gbp_band_runs")
    band, dev = band.contiguous(), band.device
    B, V, W1 = band.shape
    up, down = (torch.empty((B, V), dtype=torch.int32, device=dev) for _ in range(2))
    closed = torch.empty((B, 2, V), dtype=torch.uint8, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gbp_band_runs(B, V, W1 - 1, band.data_ptr(), threshold, up.data_ptr(), down.data_ptr(), closed.data_ptr(), _stream(dev)))
    return dict(up=up, down=down, closed_up=closed[:, 0].bool(), closed_down=closed[:, 1].bool())


BAND_BLOCK_BYTES = 2 << 30


def correlation(ens, depth_edges, chains=1, band=64, threshold=0.5, normalise=True, block=None, keep_band=True):
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
    (None: as many as keep a block's band under 2 GiB)."""
    if torch.is_tensor(ens.k) and ens.k.ndim == 2:
        check_chains(chains, ens.k.shape[1])
    z_np = centres(depth_edges)
    nd = int(z_np.size)
    W = check_band(band, nd)
    threshold = check_threshold(threshold)
    _check_block(block, "correlation")
    k, edges, sigma, B, ns, K, C, start, seg_m, seg_n, used = _check_chained(ens, chains, "correlation", "gbp_ensemble_correlation", misfit=False)
    dev = k.device
    step = max(1, BAND_BLOCK_BYTES // (nd * (W + 1) * 8)) if block is None else int(block)
    stats = torch.empty((B, 2, nd), dtype=torch.float64, device=dev)
    full = torch.empty((B, nd, W + 1), dtype=torch.float64, device=dev) if keep_band else None
    up, down = (torch.empty((B, nd), dtype=torch.int32, device=dev) for _ in range(2))
    closed = torch.empty((B, 2, nd), dtype=torch.uint8, device=dev)
    live = torch.empty((B, nd), dtype=torch.bool, device=dev)
    if B > 0:
        z = torch.as_tensor(z_np).to(dev)
        lib = _lib.load()
        work = None if keep_band else torch.empty((min(step, B), nd, W + 1), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for b0 in range(0, B, step):
                s = slice(b0, min(B, b0 + step))
                part = full[s] if keep_band else work[:s.stop - s.start]
                _lib.check(lib.gbp_ensemble_correlation(s.stop - s.start, ns, K, k[s].data_ptr(), edges[s].data_ptr(), sigma[s].data_ptr(), nd,
                                                        z.data_ptr(), 2 * C, start[s].data_ptr(), seg_m[s].data_ptr(), seg_n[s].data_ptr(), W,
                                                        int(bool(normalise)), stats[s].data_ptr(), part.data_ptr(), _stream(dev)))
                _lib.check(lib.gbp_band_runs(s.stop - s.start, nd, W, part.data_ptr(), threshold, up[s].data_ptr(), down[s].data_ptr(),
                                             closed[s].data_ptr(), _stream(dev)))
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


def main(argv=None):
    path, edges, chains, max_lag, device = parse_args(argv)
    corr = parse_correlation(argv)
    if corr is not None:
        ens = load(path, device=device)
        d = correlation(ens, edges, chains=chains, band=corr[0], threshold=corr[1])
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
