"""Pixel posteriors: every pixel of a survey raster gets a posterior of its own -- the linear pool of the hit maps of its natural
neighbours, through the cover lists a ``gridding.SibsonPlan`` already holds -- and the products are taken of THAT.

``survey_volume`` grids finished per-sounding numbers, as the reference does.  A gridded percentile is not the percentile of anything:
the Sibson average of three soundings' 95 % points is not the 95 % point of what the three say about the pixel, and the average of
three modes is a value none of them may support.  Here the order is the other way round.  The pooled maps of a whole raster cannot
exist at once (999 x 999 pixels of 250 x 440 int32 cells are 440 GB), so they are made a block of pixels at a time by one kernel
(csrc/gbp_grid.h k_sibson_pool, ``SibsonPlan.pool``) and reduced at once by the kernels that take any [B, n_value, n_depth] maps
(``hitmap.products``, ``hitmap.class_probability``).  It also gives the posterior at a place that is not a sounding, such as a
borehole (``at``).

The rule (``pool_reference`` states it in numpy; the device is held to it with ``==``): pixel p has the nearest sounding r =
index[p] and the list entries s_e = index[src_e] of the plan.  Every sounding's value axis is centred on its own prior mean, so with
u[s] = log10_shift(log_mean_prior)[s] / w, w = 2 half_width / n_value the width of a value cell, entry e is moved by d_e = (int)
rint(u[s_e] - u[r]) whole cells (round half to even, clamped to +-n_value): pooled[v, c] = sum_e maps[s_e, v - d_e, c] over the rows
inside the axis, and clipped[c] counts what fell outside.  The pixel's axis is its nearest sounding's, whose own counts are never
moved; a neighbour's counts are off by at most half a value cell plus the rounding of u.  An entry adds its sounding's counts as they
are: a sounding with more samples weighs more, and one that never burned in has an empty map and weighs nothing.  A pixel under the
plan's mask, or with an empty list, pools nothing.  There is no host fallback for the pool itself.
"""
import numpy as np
import torch

from . import _lib, gridding, hitmap
from ._args import host
from .line_products import check_classes, entropy_bits, quantiles

VARIABLES = ("mean", "median", "mode", "credible_low", "credible_high", "credible_range", "entropy", "class_probability",
             "highest_marginal", "clipped_share")


def pool_reference(index, D, dest, src, maps, pixels, u=None, max_distance_px2=np.inf):
    """(pooled int32 [P, n_value, n_depth], clipped int64 [P, n_depth]) of the rule above in numpy: ``index``, ``D`` [ny, nx] and the
    (dest, src) cover pairs of a plan over N soundings (tests/sibson_reference.py: ``nearest``, ``cover``), ``maps`` int32
    [N, n_value, n_depth], ``pixels`` a list of P flat pixel numbers (any order, repeats allowed), ``u`` float64 [N] or None (no
    shifts), ``max_distance_px2`` the plan's mask.  An entry adds its sounding's counts as they are (more samples weigh more, an empty
    map weighs nothing).  By construction pooled.sum(1) + clipped == the sum over the entries of maps[s_e].sum(0)."""
    index = np.asarray(index).reshape(-1).astype(np.int64)
    Df = np.asarray(D).reshape(-1).astype(np.float64)
    dest, src = np.asarray(dest, dtype=np.int64), np.asarray(src, dtype=np.int64)
    maps = np.asarray(maps)
    N, nv, nz = maps.shape
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    pooled = np.zeros((pixels.size, nv, nz), dtype=np.int32)
    clipped = np.zeros((pixels.size, nz), dtype=np.int64)
    for i, p in enumerate(pixels):
        if not 0 <= p < index.size:
            raise ValueError("pixel %d is outside the raster" % p)
        if Df[p] ** 2.0 + 0.25 > max_distance_px2:
            continue
        r = index[p]
        for s in index[src[np.searchsorted(dest, p, side="left"):np.searchsorted(dest, p, side="right")]]:
            d = 0 if u is None else int(np.clip(np.rint(np.float64(u[s]) - np.float64(u[r])), -nv, nv))
            m = maps[s]
            lo, hi = max(0, -d), min(nv, nv - d)                           # the source rows that stay inside the axis
            if hi > lo:
                pooled[i, lo + d:hi + d] += m[lo:hi]
            clipped[i] += m[:lo].sum(axis=0, dtype=np.int64) + m[max(hi, lo):].sum(axis=0, dtype=np.int64)
    return pooled, clipped


def at(plan, x, y):
    """The flat pixel numbers (i * nx + j, int64 [n]) of the pixels holding the coordinates ``x``, ``y`` (m): pixel (i, j) is the cell
    x_edges[j] <= x < x_edges[j + 1], y_edges[i] <= y < y_edges[i + 1], and its posterior is that of the cell's lower-left NODE, the
    point at which the plan finds every pixel's nearest sounding.  For boreholes and planned wells: ``plan.pool(maps, pixels=at(plan,
    x, y), ...)``.  A coordinate outside the raster (the last edges included) raises ValueError."""
    px, py, _, _ = gridding.pixel_coordinates(np.atleast_1d(host(x)), np.atleast_1d(host(y)), plan.x_edges, plan.y_edges)
    if not (np.all(np.isfinite(px)) and np.all(np.isfinite(py))):
        raise ValueError("the coordinates must be finite")
    j, i = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    bad = (j < 0) | (j >= plan.nx) | (i < 0) | (i >= plan.ny)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("(%g, %g) is outside the raster [%g, %g) x [%g, %g)" % (
            np.atleast_1d(host(x)).reshape(-1)[k], np.atleast_1d(host(y)).reshape(-1)[k], plan.x_edges[0],
            plan.x_edges[-1], plan.y_edges[0], plan.y_edges[-1]))
    return i * plan.nx + j


def percentile_name(p):
    return "percentile_%g" % float(p)


def _products_arguments(plan, maps, log_mean_prior, half_width, pixels, block, percentiles, credible, classes):
    """The checks of ``products`` that need no device."""
    if log_mean_prior is None or half_width is None:
        raise ValueError("pixel_posteriors.products: log_mean_prior and half_width place the value axes and are both needed")
    pix, _, lmp = gridding._pool_arguments(plan, maps, pixels, log_mean_prior, half_width, None)
    if int(block) != block or int(block) < 1:
        raise ValueError("pixel_posteriors.products: block must be a positive number of pixels")
    quantiles(percentiles, credible)
    if classes is not None:
        classes = check_classes(*classes)
    return pix, lmp, int(block), classes


def products(plan, maps, log_mean_prior, half_width, pixels=None, block=2048, percentiles=(5, 50, 95), credible=90.0, classes=None,
             depth_edges=None):
    """The products of the pixel posteriors of ``pixels`` (None: every pixel, row-major), {name: [P, n_depth]} on the plan's device:
    ``block`` pixels at a time are pooled (``SibsonPlan.pool``) into one reused buffer and reduced by ``hitmap.products`` -- mean,
    median, mode, percentile_<p>, credible_low / high / range, entropy (bits, over the pixel's own pooled map), total (int64) and s1 --
    with ``clipped_share`` = clipped / (total + clipped), the share of a column's pooled counts that fell off the pixel's value axis
    (NaN for an empty column), ``count`` [P] (the entries pooled) and ``log_mean_prior`` [P] (the pixel's axis).  With ``classes`` =
    (means, scales) (``hitmap.class_probability``) also ``class_probability`` [P, K, n_depth], ``highest_marginal`` (int32) and
    ``probability_of_highest_marginal``.  Everything is in log10 S/m on the pixel's axis, as ``hitmap.products`` of a sounding is on
    the sounding's.  A masked pixel has empty columns: what ``hitmap.products`` gives for those, and NaN shares.  The result does not
    depend on ``block``: the entropy, whose normalisation torch sums per pixel, is formed once over all P pixels."""
    out, P = {}, 0
    for p0, n, r in blocks(plan, maps, log_mean_prior, half_width, pixels, block, percentiles, credible, classes, depth_edges):
        P = n
        for k, v in r.items():
            if k not in out:
                out[k] = torch.empty((P,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            out[k][p0:p0 + v.shape[0]] = v
    if P:
        out["entropy"] = entropy(out["total"], out["s1"], maps.shape[1], half_width, depth_edges)
    return out


def entropy(total, s1, n_value, half_width, depth_edges=None):
    """The entropy (bits) ``hitmap.products`` forms from the column moments ``total`` and ``s1`` [P, n_depth], for all P pixels at once."""
    nz = total.shape[-1]
    dz = torch.ones(nz, dtype=torch.float64, device=total.device) if depth_edges is None else \
        torch.diff(torch.as_tensor(depth_edges, dtype=torch.float64, device=total.device)).abs()
    return entropy_bits(total, s1, dz * (2.0 * float(half_width) / int(n_value)))


def blocks(plan, maps, log_mean_prior, half_width, pixels=None, block=2048, percentiles=(5, 50, 95), credible=90.0, classes=None,
           depth_edges=None):
    """``products`` block by block, for results that cannot be held whole: yields (p0, P, {name: [b, ...]}) for the pixels p0 .. p0 + b
    - 1 of the list, every entry of ``products`` except ``entropy`` (form it with ``entropy`` from ``total`` and ``s1`` of all pixels:
    torch's per-pixel sum of its normalisation depends on how many pixels it is given).  The tensors of a block are its own; the
    pooled maps live in one buffer that the next block overwrites."""
    pix, lmp, block, classes = _products_arguments(plan, maps, log_mean_prior, half_width, pixels, block, percentiles, credible, classes)
    if maps.device.type != "cuda":
        raise _lib.NativeLibraryError("pixel_posteriors.products runs on the device (gbp_sibson_pool); there is no host fallback")
    dev = maps.device
    _, nv, nz = maps.shape
    P = pix.size
    max_total = int(maps.sum(dim=1, dtype=torch.int64).max()) if maps.numel() else 0
    room = max(1, min(block, P))
    buf = dict(pooled=torch.empty((room, nv, nz), dtype=torch.int32, device=dev), clipped=torch.empty((room, nz), dtype=torch.int64, device=dev))
    for p0 in range(0, P, room):
        part = plan.pool(maps, pix[p0:p0 + room], log_mean_prior=lmp, half_width=half_width, max_total=max_total, out=buf)
        r = hitmap.products(part["pooled"], part["log_mean_prior"], half_width, percentiles=percentiles, credible=credible,
                            depth_edges=depth_edges)
        del r["entropy"]
        if classes is not None:
            c = hitmap.class_probability(part["pooled"], part["log_mean_prior"], half_width, *classes)
            r.update(class_probability=c["probability"], highest_marginal=c["highest_marginal"],
                     probability_of_highest_marginal=c["probability_of_highest_marginal"])
        r["clipped_share"] = part["clipped"].to(torch.float64) / (r["total"] + part["clipped"]).to(torch.float64)
        r["count"], r["log_mean_prior"] = part["count"], part["log_mean_prior"]
        yield p0, P, r
