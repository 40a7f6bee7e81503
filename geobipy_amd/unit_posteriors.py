"""Statistics of the SAMPLED unit posteriors the device sampler accumulates (``rjmcmc_gpu.DeviceChains(units=..., first_above=...,
first_below=...)``; csrc/gbp_rjmcmc.h units_add; the host rule is ``inference.Posteriors(units=..., first=...)``).

An interval marginal (``hitmap.interval_marginals``) is the posterior of the conductivity at a depth taken at random inside a unit.
These are posteriors of properties of the unit in every sampled model, which a hit map cannot give back (it has lost the correlation
between layers): the arithmetic unit mean a = S / dz of the conductance S = int sigma dz, the harmonic unit mean h = dz / T of the
transverse resistance T = int dz / sigma -- per sample h <= a --, and the depth to the first layer at or beyond a conductivity
threshold.  ``unit_hist`` [B, Q, n_value, M] has the shape and value axis of the interval marginals, so the statistics along its value
axis are ``hitmap.products`` / ``hitmap.class_probability`` as they are (no new reduction kernel); conductance and resistance follow by
a shift: log10 S = log10 a + log10 dz, log10 T = log10 dz - log10 h (its percentiles are the harmonic mean's mirrored).

Both means are clipped to the hit map's value axis, +-``value_half_width`` decades about the chain's prior mean, like every layer's
conductivity is; being averages of layer conductivities they leave it no more often than a layer does.
"""
import numpy as np
import torch

from ._args import save_npz as save  # noqa: F401  (this module's ``save``)

KINDS = ("arithmetic", "harmonic")
STATISTICS = ("mean", "median", "mode", "credible_range")


def _pkey(p):
    return "percentile_%g" % float(p)


def _arrays(src):
    """unit_hist, first_hist, first_none (settled), log_mean_prior, unit_z, kinds, half width, depth cell of a sampler or a dict."""
    if isinstance(src, dict):
        g = src.get
        kinds = g("unit_kinds") or KINDS
        return (g("unit_hist"), g("first_hist"), g("first_none"), g("log_mean_prior"), g("unit_z"), tuple(kinds),
                g("value_half_width"), g("depth_bin_width"))
    t = src.t
    uh = src.unit_hist if t.get("unit_hist") is not None else None       # (attribute access settles the dwell times)
    fh = src.first_hist if t.get("first_hist") is not None else None
    return uh, fh, t.get("first_none"), t["log_mean_prior"], t.get("unit_z"), tuple(src.unit_kinds), src.value_half_width, src.depth_bin_width


def mirrored(percentiles):
    """The percentiles a pass must compute so that every requested one has its mirror 100 - p (the resistance's percentiles)."""
    want = [float(p) for p in percentiles]
    return tuple(want + [100.0 - p for p in want if 100.0 - p not in want])


def derive(stats, thickness, kinds=KINDS, percentiles=(5, 50, 95)):
    """The ``unit_*`` entries from the value-axis statistics of the kinds' histograms.  ``stats``: {kind: {mean, median, mode,
    credible_range, percentile_<p> ..., total}} each [N, M] (torch, any device; log10 S/m; the percentiles closed under ``mirrored``);
    ``thickness`` [N, M] = dz.  Entries are NaN where dz == 0 or nothing was accumulated.  Conductance = arithmetic + log10 dz
    (log10 S); resistance = log10 dz - harmonic (log10 ohm m^2), its percentile p from the harmonic mean's percentile 100 - p."""
    dz = torch.as_tensor(thickness, dtype=torch.float64)
    out = {}
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dz.device)
    ldz = torch.where(dz > 0.0, torch.log10(torch.where(dz > 0.0, dz, torch.ones_like(dz))), nan)
    for kind in kinds:
        s = stats[kind]
        dead = (dz <= 0.0) | (torch.as_tensor(s["total"]).to(dz.device) <= 0)
        val = lambda k: torch.where(dead, nan, torch.as_tensor(s[k], dtype=torch.float64).to(dz.device))      # noqa: E731
        for k in STATISTICS + tuple(_pkey(p) for p in percentiles):
            out["unit_%s_%s" % (kind, k)] = val(k)
        if kind == "arithmetic":
            for k in STATISTICS + tuple(_pkey(p) for p in percentiles):
                out["unit_conductance_" + k] = val(k) if k == "credible_range" else val(k) + ldz
        else:
            for k in ("mean", "median", "mode"):
                out["unit_resistance_" + k] = ldz - val(k)
            out["unit_resistance_credible_range"] = val("credible_range")
            for p in percentiles:
                out["unit_resistance_" + _pkey(p)] = ldz - val(_pkey(100.0 - float(p)))
    out["unit_thickness"] = dz
    return out


def first_depth(first_hist, first_none, depth_bin_width, percentiles=(5, 50, 95)):
    """``first_depth_median`` / ``first_depth_percentile_<p>`` [N, T] (m; centres of the depth cells: the first cell at which the
    cumulative count reaches the fraction of the samples that HAVE such a layer; NaN where none has) and ``first_probability`` =
    1 - none / samples (NaN without samples).  A cumulative sum over [N, T, n_depth]."""
    fh = torch.as_tensor(first_hist).to(torch.int64)
    none = torch.as_tensor(first_none).to(torch.int64).to(fh.device)
    cum = torch.cumsum(fh, dim=2)
    total = cum[:, :, -1]
    nan = torch.full((), float("nan"), dtype=torch.float64, device=fh.device)
    out = {}
    for name, p in [("first_depth_median", 50.0)] + [("first_depth_" + _pkey(p), float(p)) for p in percentiles]:
        need = (p * 0.01) * total.to(torch.float64)
        idx = (cum.to(torch.float64) < need[:, :, None]).sum(dim=2).clamp(max=fh.shape[2] - 1)
        out[name] = torch.where(total > 0, (idx.to(torch.float64) + 0.5) * float(depth_bin_width), nan)
    n = (total + none).to(torch.float64)
    out["first_probability"] = torch.where(n > 0, 1.0 - none.to(torch.float64) / torch.where(n > 0, n, torch.ones_like(n)), nan)
    return out


def products(chains_or_arrays, percentiles=(5, 50, 95), credible=90.0, classes=None):
    """{name: torch tensor on the sampler's device} of a sampler with unit posteriors (or a dict of its arrays: unit_hist, first_hist,
    first_none, log_mean_prior, unit_z, unit_kinds, value_half_width, depth_bin_width).  ``unit_<kind>_{mean, median, mode,
    percentile_<p>, credible_range}`` [N, M] in log10 S/m, ``unit_conductance_*`` / ``unit_resistance_*`` (see ``derive``),
    ``unit_thickness``; with ``classes`` = (means, scales) also ``unit_<kind>_class_probability`` [N, K, M] and
    ``unit_<kind>_highest_marginal``; ``first_depth_*`` / ``first_probability`` [N, T] (``first_depth``).  The histograms are viewed as
    [N Q, n_value, M] with the prior means repeated and go through ``hitmap.products`` / ``hitmap.class_probability``."""
    from . import hitmap
    uh, fh, fnone, lmp, uz, kinds, hw, dbw = _arrays(chains_or_arrays)
    out = {}
    if uh is not None:
        uh = torch.as_tensor(uh)
        B, Q, nv, M = uh.shape
        if Q != len(kinds):
            raise ValueError("unit_hist holds %d kinds, unit_kinds names %d" % (Q, len(kinds)))
        lmp_t = torch.as_tensor(lmp, dtype=torch.float64).to(uh.device)
        rows, lmp_rows = uh.reshape(B * Q, nv, M), lmp_t.repeat_interleave(Q)
        pct = mirrored(percentiles)
        if B == 0:                                      # (an empty block: the entries exist, with no rows)
            names = STATISTICS + tuple(_pkey(q_) for q_ in pct)
            p = {k: torch.empty((0, M), dtype=torch.int64 if k == "total" else torch.float64, device=uh.device) for k in names + ("total",)}
        else:
            p = hitmap.products(rows, lmp_rows, hw, percentiles=pct, credible=credible)
        stats = {kind: {k: v.view(B, Q, M)[:, q] for k, v in p.items() if k not in ("entropy", "s1")} for q, kind in enumerate(kinds)}
        z = torch.as_tensor(uz, dtype=torch.float64).to(uh.device)
        out.update(derive(stats, z[..., 1] - z[..., 0], kinds, percentiles))
        if classes is not None and B > 0:
            c = hitmap.class_probability(rows, lmp_rows, hw, *classes)
            K = c["probability"].shape[1]
            for q, kind in enumerate(kinds):
                out["unit_%s_class_probability" % kind] = c["probability"].view(B, Q, K, M)[:, q]
                out["unit_%s_highest_marginal" % kind] = c["highest_marginal"].view(B, Q, M)[:, q]
    if fh is not None:
        out.update(first_depth(fh, fnone, dbw, percentiles))
    return out
