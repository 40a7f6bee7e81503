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

There is no host fallback: both refuse tensors that are not on the device (``realisations_reference`` states the raster's rule in numpy).
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
