"""Statistics of the DATA-SPACE posteriors the device sampler accumulates (``rjmcmc_gpu.DeviceChains(data_posteriors=...)``;
csrc/gbp_rjmcmc.h data_add; the host rule is ``inference.Posteriors(data=...)``).

Does the posterior reproduce each channel, and with what spread?  ``data_hist`` [B, n_bins, N] holds, per channel, the histogram of
the residual r = (predicted - observed) / scale of every sampled model on +-``data_half_width`` scale units, ``misfit_hist``
[B, n_bins] that of log10(chi^2 / active channels) on +-``misfit_half_width`` decades; the end cells hold what lies beyond.  A hit map
cannot give these back: it has lost the correlation between layers that a prediction depends on.  ``data_hist`` has the value-major
layout of the interval marginals, so the statistics along its residual axis are ``hitmap.products`` as it is, with a prior mean of 1
(no shift) and the residual half width -- no new reduction kernel.  The shares and the misfit statistics are elementwise torch and run
on CPU tensors too.
"""
import numpy as np
import torch

from ._args import load_npz as load, save_npz as save  # noqa: F401  (this module's ``save`` and ``load``)

STATISTICS = ("mean", "median", "mode", "credible_range")


def _pkey(p):
    return "percentile_%g" % float(p)


def _arrays(src):
    """data_hist, misfit_hist (settled), observed, data_scale, data_half_width, misfit_half_width of a sampler or a dict."""
    if isinstance(src, dict):
        g = src.get
        return g("data_hist"), g("misfit_hist"), g("observed"), g("data_scale"), g("data_half_width"), g("misfit_half_width")
    t = src.t
    if t.get("data_hist") is None:
        raise ValueError("the sampler kept no data posteriors (DeviceChains(hitmap=True, data_posteriors=True))")
    dh = src.data_hist                                          # (attribute access settles the dwell times)
    return dh, t["misfit_hist"], src.observed, t["data_scale"], src.data_half_width, src.misfit_half_width


def _nan(like):
    return torch.full((), float("nan"), dtype=torch.float64, device=like.device)


def _share(part, total):
    """part / total in float64, NaN where total == 0."""
    tf = total.to(torch.float64)
    return torch.where(total > 0, part.to(torch.float64) / torch.where(total > 0, tf, torch.ones_like(tf)), _nan(total))


def _side_weights(n_bins, device, above):
    """[n_bins] weights 1 for the cells whose centre lies above (below) 0, 1/2 for a cell centred on 0 (odd axis), 0 otherwise."""
    j2 = 2 * torch.arange(n_bins, device=device) + 1               # (2 j + 1 against n_bins: the sign of the centre, in integers)
    side = (j2 > n_bins) if above else (j2 < n_bins)
    return side.to(torch.float64) + 0.5 * (j2 == n_bins).to(torch.float64)


def shares(data_hist):
    """``data_exceedance`` [B, N]: the share of samples with predicted > observed -- the cells whose centre is > 0 plus half of a cell
    centred on 0; ``data_outside``: the share in the two clamped end cells; ``data_total`` (int64): the samples.  NaN without samples."""
    h = torch.as_tensor(data_hist).to(torch.int64)
    nb = h.shape[1]
    total = h.sum(dim=1)
    w = _side_weights(nb, h.device, True)
    above = (h.to(torch.float64) * w[None, :, None]).sum(dim=1)
    return dict(data_exceedance=_share(above, total), data_outside=_share(h[:, 0] + h[:, nb - 1], total), data_total=total)


def misfit_statistics(misfit_hist, misfit_half_width, percentiles=(5, 50, 95)):
    """From ``misfit_hist`` [B, n_bins], each [B]: ``misfit_median`` / ``misfit_percentile_<p>`` as chi^2 / N_active, linear (10 to the
    centre of the first cell at which the cumulative count reaches p % of the samples), ``misfit_share_below_one`` (the cells whose
    centre is < 0 decades plus half of a cell centred on 0), ``misfit_outside`` (the two end cells), ``misfit_total``.  NaN without
    samples."""
    h = torch.as_tensor(misfit_hist).to(torch.int64)
    nb, hw = h.shape[1], float(misfit_half_width)
    cum = torch.cumsum(h, dim=1)
    total = cum[:, -1] if nb else h.sum(dim=1)
    nan = _nan(h)
    out = {}
    for name, p in [("misfit_median", 50.0)] + [("misfit_" + _pkey(p), float(p)) for p in percentiles]:
        need = (p * 0.01) * total.to(torch.float64)
        idx = (cum.to(torch.float64) < need[:, None]).sum(dim=1).clamp(max=nb - 1)
        centre = (idx.to(torch.float64) + 0.5) * (2.0 * hw / nb) - hw
        out[name] = torch.where(total > 0, torch.pow(torch.full_like(centre, 10.0), centre), nan)
    below = (h.to(torch.float64) * _side_weights(nb, h.device, False)[None, :]).sum(dim=1)
    out["misfit_share_below_one"] = _share(below, total)
    out["misfit_outside"] = _share(h[:, 0] + h[:, nb - 1], total)
    out["misfit_total"] = total
    return out


def products(chains_or_arrays, percentiles=(5, 50, 95), credible=90.0):
    """{name: torch tensor on the histograms' device} of a sampler with data posteriors (or a dict of its arrays: data_hist,
    misfit_hist, observed, data_scale, data_half_width, misfit_half_width).  [B, N]: ``data_residual_{mean, median, mode,
    credible_range, percentile_<p>}`` in scale units (``hitmap.products`` along the residual axis), ``data_predicted_{median,
    percentile_<p>}`` = observed + scale * residual, ``data_exceedance``, ``data_outside``, ``data_total`` (``shares``); NaN where a
    channel has no counts (inactive channels).  [B]: the entries of ``misfit_statistics``."""
    from . import hitmap
    dh, mh, obs, scale, hw, mhw = _arrays(chains_or_arrays)
    dh = torch.as_tensor(dh)
    B, nb, N = dh.shape
    dev = dh.device
    names = STATISTICS + tuple(_pkey(p) for p in percentiles)
    if B == 0:                                          # (an empty block: the entries exist, with no rows)
        p = {k: torch.empty((0, N), dtype=torch.float64, device=dev) for k in names}
    else:
        p = hitmap.products(dh, torch.zeros(B, dtype=torch.float64, device=dev), float(hw), percentiles=percentiles, credible=credible)
    out = shares(dh)
    dead = out["data_total"] <= 0
    nan = _nan(dh)
    for k in names:
        out["data_residual_" + k] = torch.where(dead, nan, p[k].to(torch.float64))
    obs = torch.as_tensor(obs, dtype=torch.float64).to(dev)
    scale = torch.as_tensor(scale, dtype=torch.float64).to(dev)
    for k in ("median",) + tuple(_pkey(p_) for p_ in percentiles):
        out["data_predicted_" + k] = obs + scale * out["data_residual_" + k]
    out.update(misfit_statistics(torch.as_tensor(mh).to(dev), mhw, percentiles))
    return out
