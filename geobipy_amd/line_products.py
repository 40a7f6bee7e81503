"""Posterior line products of a flight line's results container: the mean, median and mode models, percentiles and the credible interval,
entropy, opacity, depth of investigation (DOI) and interface probability -- what the reference's ``Inference2D`` derives from the hit maps
(inversion/Inference2D.py: compute_mean/median/mode_parameter, percentile, credible_interval, compute_opacity, compute_doi, entropy,
interface_probability) -- and, for K classes defined in log10 conductivity, the class (lithology) probabilities of every depth cell and
the most probable class (Inference2D.compute_probability, highestMarginal, probability_of_highest_marginal; Minsley, Foks & Bedrosian 2020).

The work splits in two.  Per sounding, one streaming kernel reduces every (sounding, depth cell) column of the int32 hit maps to a few
moments -- total, sum c ln c, the mode's cell, the quantiles' cells, the mean (csrc/gbp_hitmap.h: k_hitmap_products, through
``hitmap.products``); the maps go up a block at a time and never leave the device.  With classes, a second kernel reduces the same
uploaded block to the K class probabilities (k_hitmap_classes, through ``hitmap.class_probability``).  Per line, the small functions
below finish on [N, n_depth] arrays: they run on whichever device their tensors are on (the CPU tier tests them without a GPU).
Everything is log10 conductivity (S/m) except entropy (bits), opacity and probabilities (0 - 1) and the depths (m).

    python -m geobipy_amd.line_products <container or directory> [--credible 90] [--doi 67] [--percentiles 5 50 95]
                                        [--class-means M1 M2 ... --class-scales S1 S2 ...] [--elevation-axis DZ [TOP BOTTOM]]
                                        [--depth-intervals E0 E1 ... | --elevation-intervals E0 E1 ...]
                                        [--mixtures [KMAX] [--mixture-iterations N]]

writes ``<line>.products.npz`` next to each ``<line>.h5`` / ``<line>.results.npz``.  The class means and scales (standard deviations)
are in log10 S/m; they come together, 1 to 16 of each.  With ``--elevation-axis`` the per-depth-cell products also go onto a regular
elevation axis (``on_elevation``, ``elevation.regular_axis``), written to ``<line>.products_elevation.npz`` beside the first file.
With ``--depth-intervals`` / ``--elevation-intervals`` the file also holds the products of the units between those edges (``interval_*``:
the statistics of each unit's marginal posterior, ``from_results(intervals=...)``, geobipy_amd/intervals.py).  With ``--mixtures`` it
holds the local mixture fit of every depth cell's posterior (``mixture_*``, geobipy_amd/mixtures.py), from which
``python -m geobipy_amd.mixtures`` derives global classes for ``--class-means`` / ``--class-scales``.
"""
import argparse
import glob
import math
import os
import sys

import numpy as np
import torch

LN10 = 2.302585092994046
MAX_QUANTILES = 8
MAX_CLASSES = 16

VALUES = "/model/values/posterior"            # the conductivity-depth hit maps [N, n_value, n_depth] and their mesh
INTERFACES = "/model/mesh/y/edges/posterior"  # the interface-depth hit counts [N, n_depth]


def _t(x, dtype=torch.float64):
    return x.to(dtype) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=dtype)


def credible_bounds(credible):
    """(low, high) percents of the ``credible`` % interval: 0.5 min(c, 100 - c) and 100 minus it (mesh/Mesh.py:58-78)."""
    lo = 0.5 * min(float(credible), 100.0 - float(credible))
    return lo, 100.0 - lo


def quantiles(percentiles=(5, 50, 95), credible=90.0):
    """(q, {percent: position in q}, (low, high) positions of the credible bounds in q): the distinct quantiles in (0, 1), at most 8,
    one kernel pass needs for the requested percentiles, the median and the ``credible`` % interval.  The two forms differ where a
    cumulative share falls EXACTLY on a quantile, as the reference's do: a percentile p is the quantile p / 100, correctly rounded
    (the 0.05 / 0.5 / 0.95 of ``hitmap.statistics``, and the reference's ``Histogram.percentile``, whose shares are cumulative sums of
    the pmf that round to the same side on such ties), a credible bound b is b * 0.01 (``Histogram.credible_range`` cumulates the
    integer counts against r_[b, 100 - b] * 0.01, mesh/Mesh.py:58-78: 95 * 0.01 = 0.9500000000000001).  The fixture
    tests/golden/line_products.npz holds such ties."""
    lo, hi = credible_bounds(credible)
    pct = sorted({float(p) for p in percentiles} | {50.0})
    if not all(0.0 < p < 100.0 for p in pct) or not 0.0 < lo < 100.0:
        raise ValueError("percentiles and the credible interval must lie in (0, 100): %r, %r" % (pct, credible))
    q = sorted({p / 100.0 for p in pct} | {lo * 0.01, hi * 0.01})
    if len(q) > MAX_QUANTILES:
        raise ValueError("at most %d distinct quantiles (percentiles + median + credible bounds) per pass, got %d" % (MAX_QUANTILES, len(q)))
    return q, {p: q.index(p / 100.0) for p in pct}, (q.index(lo * 0.01), q.index(hi * 0.01))


def log10_shift(log_mean_prior):
    """The prior mean in log10, ln / 2.302585092994046 as k_hitmap_stats divides it ([B] float64 on the input's device; the division is
    done by numpy, correctly rounded, where torch's division of a device tensor by a scalar multiplies by the reciprocal)."""
    dev = log_mean_prior.device if torch.is_tensor(log_mean_prior) else torch.device("cpu")
    lmp = log_mean_prior.detach().cpu().numpy() if torch.is_tensor(log_mean_prior) else np.asarray(log_mean_prior)
    return torch.as_tensor(np.asarray(lmp, dtype=np.float64) / LN10).to(dev)


def value_centres(idx, n_value, half_width, shift):
    """log10 conductivity of value cell ``idx``: ((idx + 0.5) / n_value) 2 half_width - half_width + shift, the centre expression of
    k_hitmap_stats evaluated once per cell by numpy and gathered, so that a percentile here has the bits of ``hitmap.statistics``'s on
    any device (``shift`` from ``log10_shift``, broadcast against ``idx``)."""
    idx = idx if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx))
    table = ((np.arange(int(n_value), dtype=np.float64) + 0.5) / float(n_value)) * (2.0 * float(half_width)) - float(half_width)
    c = torch.as_tensor(table).to(idx.device)[idx.long()]
    return c + _t(shift).to(c.device)


def entropy_bits(total, s1, cell_area):
    """Entropy in bits per depth cell from the column moments [B, n_depth] (``total`` = S0 = sum_v c, ``s1`` = S1 = sum_v c ln c) and the
    cell areas dvalue x ddepth [n_depth], under the reference's normalisation (``Histogram.entropy`` over ``Histogram.pdf``,
    statistics/Histogram.py:34-41, 129-148): p = c / Z with Z = sum over the sounding's cells of area c, so
    H_z = -sum_v p log2 p = -(S1_z - S0_z ln Z) / (Z ln 2).  An empty sounding (Z = 0) has entropy 0, as the reference's zero pdf."""
    S0 = _t(total)
    S1 = _t(s1).to(S0.device)
    Z = (S0 * _t(cell_area).to(S0.device)).sum(dim=-1, keepdim=True)
    Zs = torch.where(Z > 0, Z, torch.ones_like(Z))
    H = -(S1 - S0 * torch.log(Zs)) / (Zs * math.log(2.0))
    return torch.where(Z > 0, H, torch.zeros_like(H))


def transparency(credible_range):
    """The reference's transparency (statistics/Histogram.py:509-542) over a whole line [N, n_depth]: the credible range normalised by
    its nanmin / nanmax over all soundings and depth cells (shifted only, when they are equal), NaN -> 1."""
    r = _t(credible_range)
    fin = r[~torch.isnan(r)]
    if fin.numel() == 0:
        return torch.ones_like(r)
    mn, mx = fin.min(), fin.max()
    t = (r - mn) / (mx - mn) if float(mx - mn) > 0.0 else r - mn
    return torch.where(torch.isnan(t), torch.ones_like(t), t)


def opacity(credible_range):
    """1 - ``transparency``: narrow credible intervals are opaque (statistics/Histogram.py:330-354)."""
    return 1.0 - transparency(credible_range)


def doi_index(opac, percent=67.0):
    """The reference's DOI walk (inversion/Inference2D.py:493-535) per sounding of opacity [N, n_depth]: from the deepest cell up while
    the opacity is below percent / 100, stopping at cell 0 -- the deepest cell whose opacity reaches the level, else 0 (int64 [N])."""
    if not 0.0 < float(percent) < 100.0:
        raise ValueError("the DOI percent must lie in (0, 100)")
    o = _t(opac)
    keep = ~(o < 0.01 * float(percent))                               # (a NaN stops the walk, as in the reference's loop)
    keep[:, 0] = True
    j = torch.arange(o.shape[-1], device=o.device).expand_as(o)
    return torch.where(keep, j, torch.zeros_like(j)).max(dim=-1).values


def interface_pdf(counts, x_edges, depth_edges):
    """``Histogram.pdf`` (statistics/Histogram.py:34-41) of the line's interface-depth histogram [N, n_depth] over its 2-D mesh (the
    container's sounding axis x by depth): counts / sum(area counts) with area = |dx| |ddepth|; all zero when nothing was counted.
    With one sounding, the pdf over its 1-D depth mesh."""
    c = _t(counts)
    area = torch.outer(torch.diff(_t(x_edges)).abs(), torch.diff(_t(depth_edges)).abs()).to(c.device)
    if float(c.max()) <= 0:
        return torch.zeros_like(c)
    return c / (area * c).sum()


def _uniform_half_width(edges):
    e = np.asarray(edges, dtype=np.float64)
    hw = float(e[-1])
    n = e.size - 1
    step = 2.0 * hw / n
    if abs(e[0] + hw) > 1e-9 * max(1.0, hw) or np.abs(np.diff(e) - step).max() > 1e-9 * max(1.0, step):
        raise ValueError("the value axis of %s must be uniform and symmetric about the prior mean (edges %r .. %r)" % (VALUES, e[0], e[-1]))
    return hw


def _key(arrays, *names):
    for n in names:
        if n in arrays:
            return np.asarray(arrays[n])
    return None


def check_classes(means, scales):
    """(means, scales) as float64 arrays of 1 to 16 classes in log10 S/m: equal lengths, finite means, finite positive scales."""
    mu = np.asarray(means, dtype=np.float64).reshape(-1)
    sd = np.asarray(scales, dtype=np.float64).reshape(-1)
    if mu.size != sd.size or not 1 <= mu.size <= MAX_CLASSES:
        raise ValueError("classes: 1 to %d means and as many scales, got %d and %d" % (MAX_CLASSES, mu.size, sd.size))
    if not np.all(np.isfinite(mu)) or not np.all(np.isfinite(sd) & (sd > 0.0)):
        raise ValueError("classes: the means must be finite and the scales finite and positive")
    return mu, sd


INTERVAL_DROPPED = ("entropy", "s1")          # (the reference's density is over the sounding's 2-D mesh: not defined for a unit)


MIXTURE_OPTIONS = ("max_components", "n_iter", "reg", "epsilon", "mu")
MIXTURE_ENTRIES = (("n", "n_components"), ("weight", "weight"), ("mean", "mean"), ("sd", "sd"), ("misfit", "misfit"), ("ll_change", "ll_change"))


def check_mixtures(options, n_value, half_width):
    """The ``mixtures=`` options of ``from_results`` as the keyword arguments of ``mixtures.fit``, checked (True / an empty dict: the
    defaults)."""
    from . import mixtures as mx
    o = {} if options is True else dict(options)
    if set(o) - set(MIXTURE_OPTIONS):
        raise ValueError("mixtures: unknown options %r (known: %s)" % (sorted(set(o) - set(MIXTURE_OPTIONS)), ", ".join(MIXTURE_OPTIONS)))
    K, n_iter, reg = mx.check_arguments(n_value, half_width, o.get("max_components", 3), o.get("n_iter", 50), o.get("reg"))
    eps, mu = float(o.get("epsilon", 0.05)), float(o.get("mu", 0.1))
    if not (math.isfinite(eps) and math.isfinite(mu) and eps >= 0.0 and mu >= 0.0):
        raise ValueError("mixtures: epsilon and mu must be finite and not negative")
    return dict(max_components=K, n_iter=n_iter, reg=reg, epsilon=eps, mu=mu)


def mixture_products(hm, lmp, half_width, options, prefix="mixture_"):
    """The ``mixture_*`` entries of a block of hit maps (or int64 interval marginals) on the device: ``mixtures.fit`` under ``options``
    (``check_mixtures``) -> <prefix>n [B, n_depth] (int32), <prefix>weight / mean / sd [B, Kmax, n_depth], <prefix>misfit [B, 2,
    n_depth] and <prefix>ll_change [B, n_depth]."""
    from . import mixtures as mx
    f = mx.fit(hm, lmp, half_width, **options)
    return {prefix + a: f[b] for a, b in MIXTURE_ENTRIES}


def interval_products(hm, lmp, half_width, lo, hi, percentiles=(5, 50, 95), credible=90.0, classes=None, mixtures=None):
    """The ``interval_*`` entries of a block of hit maps on the device: ``hitmap.interval_marginals`` over the ranges ``lo`` / ``hi``
    [B, M], then ``hitmap.products`` (and ``hitmap.class_probability`` for ``classes`` = (means, scales)) along the value axis of the
    int64 marginals [B, n_value, M]: mean, median, mode, percentile_<p>, credible_low / high / range, total (int64) [B, M] and, with
    classes, class_probability [B, K, M], highest_marginal, probability_of_highest_marginal; float entries NaN where a range has no
    cells.  With ``mixtures`` (the options of ``check_mixtures``) also the local mixture fits of the marginals, interval_mixture_*
    (``mixture_products``).  Torch tensors on the maps' device."""
    from . import hitmap
    marg = hitmap.interval_marginals(hm, lo, hi)
    nz = hm.shape[2]
    empty = (torch.as_tensor(hi).clamp(0, nz) <= torch.as_tensor(lo).clamp(0, nz)).to(marg.device)      # (as the kernel clamps them)
    empty = empty[None, :].expand(marg.shape[0], -1) if empty.ndim == 1 else empty
    p = hitmap.products(marg, lmp, half_width, percentiles=percentiles, credible=credible)
    out = {"interval_" + k: v for k, v in p.items() if k not in INTERVAL_DROPPED}
    if classes is not None:
        c = hitmap.class_probability(marg, lmp, half_width, *classes)
        out.update(interval_class_probability=c["probability"], interval_highest_marginal=c["highest_marginal"],
                   interval_probability_of_highest_marginal=c["probability_of_highest_marginal"])
    if mixtures is not None:
        out.update(mixture_products(marg, lmp, half_width, mixtures, prefix="interval_mixture_"))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=marg.device)
    for k, v in out.items():
        if v.dtype.is_floating_point:
            out[k] = torch.where(empty[:, None, :] if v.ndim == 3 else empty, nan, v)
    return out


def from_results(path, device=None, block=4096, percentiles=(5, 50, 95), credible=90.0, doi=67.0, classes=None, intervals=None, mixtures=None):
    """{name: numpy array} of the line products of the results container at ``path`` (``<line>.h5`` or the ``.results[.npz]`` stand-in,
    read through ``hdf.load_results``; the reference's own files where they hold this layout).  The hit maps go to ``device`` (default
    cuda:0) ``block`` soundings at a time.  Per sounding [N, n_depth] (log10 S/m): mean, median, mode, percentile_<p>, credible_low /
    high / range; entropy (bits); per line: transparency and opacity at ``credible`` %, doi_index / doi_depth at ``doi`` % and
    interface_probability [N, n_depth].

    The reference's DOI is ``mesh.y_centres`` at the index of the walk, and its mesh flips depth to height relative to the data's
    elevation (Inference2D.mesh: y edges negated, relative_to = elevation), so y_centres = elevation - depth centre.  ``doi_depth`` is
    the depth centre below the surface (m, positive down); ``doi_elevation`` = elevation - doi_depth is the reference's value, present
    where the container has /data/elevation.

    ``classes`` = (means, scales), 1 to 16 classes in log10 S/m (scales: standard deviations; ``hitmap.class_probability``), adds
    ``class_probability`` [N, K, n_depth] (the layout of the reference's ``probabilities``), ``highest_marginal`` [N, n_depth] (int32),
    ``probability_of_highest_marginal`` [N, n_depth], ``class_means`` and ``class_scales``, from the blocks the products were computed
    on (no second upload).  The reference takes its argmax over the last axis of a [N, K, n_depth] array in Inference3D but over the
    class axis in Inference2D; here it is over the class axis.

    ``intervals`` = a spec (``intervals.check_spec``: {"kind": "depth", "edges": [...]}, {"kind": "pairs", "pairs": [[d0, d1], ...]},
    {"kind": "elevation", "edges": [...]} under the container's /data/elevation, or {"kind": "horizons", "top": ..., "bottom": ...})
    adds the products of M depth or elevation UNITS, each the statistic of the unit's marginal posterior -- the hit map's counts summed
    over the unit's depth cells (``hitmap.interval_marginals``), not a mean over per-cell products: ``interval_mean`` / ``_median`` /
    ``_mode`` / ``_percentile_<p>`` / ``_credible_low`` / ``_high`` / ``_range`` [N, M] (NaN where a unit has no cells under a sounding),
    ``interval_total`` (int64) and ``interval_cells`` (int32) [N, M], ``interval_lo`` / ``interval_hi`` (the cell ranges), with classes
    ``interval_class_probability`` [N, K, M], ``interval_highest_marginal`` and ``interval_probability_of_highest_marginal``, and the
    spec itself (``interval_kind``, ``interval_edges`` / ``interval_pairs`` / ``interval_top``, ``interval_bottom``).  The ranges are
    computed once per line on the host; the marginals come from the blocks the products are computed on.  Entropy, opacity and DOI are
    not defined for units.

    ``mixtures`` = a dict of options (``max_components`` 1 .. 4, default 3; ``n_iter``, ``reg``, ``epsilon``, ``mu``: ``mixtures.fit``;
    True for the defaults) adds the local mixture fit of every column from the same uploaded blocks (``hitmap.mixture``, DESIGN.md
    3.16): ``mixture_n`` [N, n_depth] (int32, the number of components the stopping rule keeps; 0 for an empty column),
    ``mixture_weight`` / ``mixture_mean`` / ``mixture_sd`` [N, Kmax, n_depth] (sorted by mean, NaN beyond mixture_n; means in log10
    S/m), ``mixture_misfit`` [N, 2, n_depth] and ``mixture_ll_change`` [N, n_depth] (the log-likelihood's change over the last
    iteration: whether n_iter was enough).  With ``intervals`` also ``interval_mixture_*`` [N, Kmax, M], the fits of the units'
    marginal posteriors.  ``mixtures.global_classes`` turns the lines' fits into classes."""
    from . import hdf, hitmap
    from . import intervals as iv
    if not 0.0 < float(credible) < 100.0:
        raise ValueError("credible must lie in (0, 100)")
    if classes is not None:
        cmeans, cscales = check_classes(*classes)
    arrays, _ = hdf.load_results(path)
    hm_all = _key(arrays, VALUES + "/values/data", VALUES + "/values")
    if hm_all is None or hm_all.ndim != 3:
        raise ValueError("%s holds no conductivity-depth hit maps [N, n_value, n_depth] at %s" % (path, VALUES))
    v_edges = _key(arrays, VALUES + "/mesh/y/edges/data")
    d_edges = _key(arrays, VALUES + "/mesh/z/edges/data")
    rel = _key(arrays, VALUES + "/mesh/y/relative_to/data")
    N, nv, nz = hm_all.shape
    if v_edges is None or d_edges is None or v_edges.size != nv + 1 or d_edges.size != nz + 1:
        raise ValueError("%s: the hit maps' mesh (%s/mesh/y and /z edges) does not match their shape %r" % (path, VALUES, hm_all.shape))
    hw = _uniform_half_width(v_edges)
    if mixtures is not None:
        mixtures = check_mixtures(mixtures, nv, hw)
    rel = np.zeros(N) if rel is None else np.broadcast_to(np.asarray(rel, dtype=np.float64).reshape(-1), (N,))
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    elev = _key(arrays, "/data/elevation/data", "/data/elevation")
    if intervals is not None:
        spec = iv.check_spec(intervals)
        surface = None if elev is None or np.asarray(elev).size != N else np.asarray(elev, dtype=np.float64).reshape(-1)
        rng = iv.ranges(spec, d_edges, N, surface=surface)
    parts = []
    for b0 in range(0, N, int(block)):
        b1 = min(N, b0 + int(block))
        hm = torch.as_tensor(np.ascontiguousarray(hm_all[b0:b1], dtype=np.int32)).to(dev)
        lmp = torch.as_tensor(rel[b0:b1] * LN10, dtype=torch.float64, device=dev)
        p = hitmap.products(hm, lmp, hw, percentiles=percentiles, credible=credible, depth_edges=d_edges)
        if intervals is not None:
            p.update(interval_products(hm, lmp, hw, torch.as_tensor(rng.lo[b0:b1]), torch.as_tensor(rng.hi[b0:b1]), percentiles=percentiles,
                                       credible=credible, classes=None if classes is None else (cmeans, cscales), mixtures=mixtures))
        if mixtures is not None:
            p.update(mixture_products(hm, lmp, hw, mixtures))
        if classes is not None:
            c = hitmap.class_probability(hm, lmp, hw, cmeans, cscales)
            p.update(class_probability=c["probability"], highest_marginal=c["highest_marginal"],
                     probability_of_highest_marginal=c["probability_of_highest_marginal"])
        parts.append({k: v.cpu() for k, v in p.items()})
    keys = parts[0].keys() if parts else []
    out = {k: torch.cat([p_[k] for p_ in parts]).numpy() for k in keys}
    out.pop("total", None)
    out.pop("s1", None)
    cr = torch.as_tensor(out["credible_range"]) if N else torch.zeros((0, nz), dtype=torch.float64)
    t = transparency(cr) if N else cr
    out["transparency"] = t.numpy()
    out["opacity"] = (1.0 - t).numpy()
    j = doi_index(1.0 - t, doi).numpy() if N else np.zeros(0, dtype=np.int64)
    depth_centres = 0.5 * (d_edges[1:] + d_edges[:-1])
    out["doi_index"] = j
    out["doi_depth"] = depth_centres[j]
    if elev is not None and np.asarray(elev).size == N:
        out["doi_elevation"] = np.asarray(elev, dtype=np.float64).reshape(-1) - out["doi_depth"]
    ic = _key(arrays, INTERFACES + "/values/data")
    ix = _key(arrays, INTERFACES + "/mesh/x/edges/data")
    iz = _key(arrays, INTERFACES + "/mesh/y/edges/data")
    if ic is not None and ix is not None and iz is not None and ic.ndim == 2 and ic.shape[0] == N:
        out["interface_probability"] = interface_pdf(ic, ix, iz).numpy()
        out["interface_depth_edges"] = np.asarray(iz, dtype=np.float64)
    out["depth_edges"] = np.asarray(d_edges, dtype=np.float64)
    out["depth_centres"] = depth_centres
    fid = _key(arrays, "/data/fiducial/data", "/data/fiducial")
    if fid is not None:
        out["fiducial"] = np.asarray(fid)
    out["credible"], out["doi_percent"] = np.float64(credible), np.float64(doi)
    if classes is not None:
        if not N:
            K = cmeans.size
            out.update(class_probability=np.zeros((0, K, nz)), highest_marginal=np.zeros((0, nz), dtype=np.int32),
                       probability_of_highest_marginal=np.zeros((0, nz)))
        out["class_means"], out["class_scales"] = cmeans, cscales
    if mixtures is not None and not N:
        cells = [("mixture_", nz)] + ([("interval_mixture_", iv.n_intervals(spec))] if intervals is not None else [])
        for prefix, n in cells:
            out[prefix + "n"] = np.zeros((0, n), dtype=np.int32)
            out.update({prefix + k: np.zeros((0, mixtures["max_components"], n)) for k in ("weight", "mean", "sd")})
            out[prefix + "misfit"], out[prefix + "ll_change"] = np.zeros((0, 2, n)), np.zeros((0, n))
    if intervals is not None:
        if not N:
            M = iv.n_intervals(spec)
            names = ["mean", "median", "mode", "credible_low", "credible_high", "credible_range"] + ["percentile_%g" % float(p) for p in percentiles]
            out.update({"interval_" + k: np.zeros((0, M)) for k in names})
            out["interval_total"] = np.zeros((0, M), dtype=np.int64)
            if classes is not None:
                out.update(interval_class_probability=np.zeros((0, cmeans.size, M)), interval_highest_marginal=np.zeros((0, M), dtype=np.int32),
                           interval_probability_of_highest_marginal=np.zeros((0, M)))
        out["interval_cells"], out["interval_lo"], out["interval_hi"] = rng.n_cells, rng.lo, rng.hi
        out.update(iv.describe(spec))
    return out


def on_elevation(products, surface, edges=None, levels=None, device=None):
    """The per-depth-cell entries of ``products`` (``from_results``) on an elevation axis (``elevation.resample``, on ``device``, default
    cuda:0): every entry shaped [N, n_depth] or [N, K, n_depth] over ``products['depth_edges']`` becomes [N, E] / [N, K, E] -- the mean
    over each cell of the ascending ``edges`` [E + 1], or the value at each of ``levels`` [E]; exactly one of the two.  ``surface`` [N]:
    the soundings' surface elevation (the container's /data/elevation).  Integer entries (class indices: ``highest_marginal``) are never
    averaged: with ``edges`` they are taken at the centre of each cell.  Everything else (the per-sounding and per-line entries, the
    depth axes, the ``interval_*`` entries, which are over units and not over depth cells however many there are, the ``mixture_*``
    entries, whose components have no identity from one depth cell to the next that a mean over cells could keep,
    ``interface_probability`` where it has a depth mesh of its own) passes through, and the result also carries
    ``elevation_edges`` (and ``elevation_centres``) or ``elevation_levels``, and ``surface``."""
    from . import _lib, elevation
    mode, axis, _ = elevation.check_axis(levels=levels, edges=edges)
    if "depth_edges" not in products:
        raise ValueError("the products hold no depth_edges")
    d_edges = elevation.check_depth_edges(products["depth_edges"])
    nz = d_edges.size - 1
    s = np.asarray(surface, dtype=np.float64).reshape(-1)
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    if dev.type != "cuda":
        raise _lib.NativeLibraryError("line_products.on_elevation runs on the device (gbp_elevation_resample); there is no host fallback")
    centres = 0.5 * (axis[1:] + axis[:-1]) if mode == elevation.INTERVALS else None
    out = {}
    for k, v in products.items():
        a = np.asarray(v)
        own_mesh = k == "interface_probability" and not np.array_equal(np.asarray(products.get("interface_depth_edges", d_edges)), d_edges)
        if (k.startswith(("interval_", "mixture_")) or a.ndim not in (2, 3) or a.shape[-1] != nz or a.shape[0] != s.size or a.size == 0 or own_mesh
                or a.dtype.kind not in "fiub"):                             # (interval_*: over units, not depth cells, whatever their count)
            out[k] = v
            continue
        t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        if a.dtype.kind == "f":
            r = elevation.resample(t.to(torch.float64), s, d_edges, levels=levels, edges=edges)
        else:
            r = elevation.resample(t, s, d_edges, levels=axis if centres is None else centres)
        out[k] = r.cpu().numpy()
    if centres is None:
        out["elevation_levels"] = axis
    else:
        out["elevation_edges"], out["elevation_centres"] = axis, centres
    out["surface"] = s
    return out


def save(products, path):
    """Write ``products`` ({name: array}) to ``path`` (``<line>.products.npz``) with np.savez_compressed; returns the path."""
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in products.items()})
    return path


_SUFFIXES = (".results.npz", ".results", ".hdf5", ".h5")


def output_path(container):
    """``<line>.products.npz`` next to the container ``<line>.h5`` / ``<line>.hdf5`` / ``<line>.results[.npz]``."""
    for s in _SUFFIXES:
        if container.endswith(s):
            return container[:-len(s)] + ".products.npz"
    return container + ".products.npz"


def elevation_output_path(container):
    """``<line>.products_elevation.npz`` next to the container."""
    return output_path(container)[:-len(".products.npz")] + ".products_elevation.npz"


def containers(path):
    """The results containers at ``path``: the file itself, or a directory's ``*.h5`` / ``*.hdf5`` / ``*.results.npz``, sorted."""
    if os.path.isdir(path):
        found = set()
        for pat in ("*.h5", "*.hdf5", "*.results.npz"):
            found.update(glob.glob(os.path.join(path, pat)))
        return sorted(found)
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return [path]


def parser():
    ap = argparse.ArgumentParser(prog="python -m geobipy_amd.line_products",
                                 description="Posterior line products (mean, median, mode, percentiles, credible range, entropy, opacity, "
                                             "DOI, interface probability and, with --class-means / --class-scales, class probabilities and "
                                             "the most probable class) of GeoBIPy results containers, written to <line>.products.npz.")
    ap.add_argument("paths", nargs="+", help="results containers (<line>.h5, <line>.results.npz) or directories holding them")
    ap.add_argument("--credible", type=float, default=90.0, help="credible interval of the opacity, percent (default 90)")
    ap.add_argument("--doi", type=float, default=67.0, help="opacity level of the depth of investigation, percent (default 67)")
    ap.add_argument("--percentiles", type=float, nargs="+", default=[5.0, 50.0, 95.0], help="percentiles to write (default 5 50 95)")
    ap.add_argument("--class-means", type=float, nargs="+", default=None, metavar="M",
                    help="means of 1 to 16 classes (lithologies) in log10 S/m; with --class-scales")
    ap.add_argument("--class-scales", type=float, nargs="+", default=None, metavar="S",
                    help="standard deviations of the classes in log10 S/m, one per mean, positive")
    ap.add_argument("--elevation-axis", type=float, nargs="+", default=None, metavar="DZ [TOP BOTTOM]",
                    help="also write <line>.products_elevation.npz: the per-depth-cell products averaged over the cells of a regular "
                         "elevation axis of DZ m, from BOTTOM to TOP (default: everything the line's soundings reach), snapped outward "
                         "to multiples of DZ")
    add_interval_arguments(ap)
    ap.add_argument("--mixtures", type=int, nargs="?", const=3, default=None, metavar="KMAX",
                    help="also the local mixture fit of every depth cell's posterior (and of every unit's, with intervals): up to KMAX "
                         "Gaussians, 1 to 4 (default 3), written as mixture_* entries")
    ap.add_argument("--mixture-iterations", type=int, default=None, metavar="N", help="EM iterations of --mixtures (default 50)")
    ap.add_argument("--block", type=int, default=4096, help="soundings per upload (default 4096)")
    ap.add_argument("--device", default=None, help="torch device of the kernel (default cuda:0)")
    return ap


def add_interval_arguments(ap):
    """``--depth-intervals`` / ``--elevation-intervals E0 E1 ...`` of the command lines."""
    ap.add_argument("--depth-intervals", type=float, nargs="+", default=None, metavar="E",
                    help="also the products of the depth units between these edges (m below the surface; at least two, ascending): "
                         "each the statistic of the unit's marginal posterior, written as interval_* entries")
    ap.add_argument("--elevation-intervals", type=float, nargs="+", default=None, metavar="E",
                    help="the same for the elevation units between these edges (m; at least two, ascending; unit 0 the lowest), under "
                         "each sounding's own surface elevation")


def interval_arguments(ap, a, selectors):
    """The interval spec of parsed arguments ``a`` (None without one), checked: one of the two flags, none of ``selectors`` (names of
    the depth / elevation selectors of the command line) beside it, at least two finite ascending edges."""
    from . import intervals as iv
    given = [(n, v) for n, v in (("depth", a.depth_intervals), ("elevation", a.elevation_intervals)) if v is not None]
    if not given:
        return None
    if len(given) > 1:
        ap.error("--depth-intervals and --elevation-intervals exclude each other")
    for name in selectors:
        if getattr(a, name.lstrip("-").replace("-", "_")) is not None:
            ap.error("--%s-intervals and %s exclude each other" % (given[0][0], name))
    try:
        return dict(kind=given[0][0], edges=iv.edges_argument(given[0][1]))
    except ValueError as e:
        ap.error("--%s-intervals: %s" % (given[0][0], e))


def parse_args(argv=None):
    """The command line's arguments, checked: percents in (0, 100), at most 8 distinct quantiles per pass, a positive block, class means
    and scales together, 1 to 16 of each, equal counts, positive scales, --elevation-axis DZ or DZ TOP BOTTOM with DZ > 0 and BOTTOM < TOP."""
    ap = parser()
    a = ap.parse_args(argv)
    for name, v in (("--credible", a.credible), ("--doi", a.doi)):
        if not 0.0 < v < 100.0:
            ap.error("%s must lie in (0, 100), got %g" % (name, v))
    if any(not 0.0 < p < 100.0 for p in a.percentiles):
        ap.error("--percentiles must lie in (0, 100)")
    try:
        quantiles(a.percentiles, a.credible)
    except ValueError as e:
        ap.error(str(e))
    if a.block < 1:
        ap.error("--block must be positive")
    if (a.class_means is None) != (a.class_scales is None):
        ap.error("--class-means and --class-scales come together")
    if a.class_means is not None:
        try:
            check_classes(a.class_means, a.class_scales)
        except ValueError as e:
            ap.error("--class-means / --class-scales: " + str(e))
    if a.elevation_axis is not None:
        try:
            elevation_axis_arguments(a.elevation_axis)
        except ValueError as e:
            ap.error("--elevation-axis: " + str(e))
    a.intervals = interval_arguments(ap, a, ("--elevation-axis",))
    if a.mixtures is None and a.mixture_iterations is not None:
        ap.error("--mixture-iterations comes with --mixtures")
    if a.mixtures is not None:
        if not 1 <= a.mixtures <= 4:
            ap.error("--mixtures KMAX must lie in 1 .. 4")
        n_iter = 50 if a.mixture_iterations is None else a.mixture_iterations
        if not 1 <= n_iter <= 10000:
            ap.error("--mixture-iterations must lie in 1 .. 10000")
        a.mixtures = dict(max_components=a.mixtures, n_iter=n_iter)
    return a


def elevation_axis_arguments(values):
    """(dz, top, bottom) of the command lines' ``--elevation-axis DZ [TOP BOTTOM]`` (top and bottom None where left out), checked."""
    v = [float(x) for x in values]
    if len(v) not in (1, 3):
        raise ValueError("DZ, or DZ TOP BOTTOM")
    if not all(np.isfinite(v)) or not v[0] > 0.0:
        raise ValueError("DZ must be positive, everything finite")
    if len(v) == 3 and not v[2] < v[1]:
        raise ValueError("BOTTOM must lie below TOP")
    return (v[0], None, None) if len(v) == 1 else (v[0], v[1], v[2])


def main(argv=None):
    a = parse_args(argv)
    files = [f for p in a.paths for f in containers(p)]
    if not files:
        print("no results containers under %s" % " ".join(a.paths), file=sys.stderr)
        return 1
    for f in files:
        classes = None if a.class_means is None else (a.class_means, a.class_scales)
        out = from_results(f, device=a.device, block=a.block, percentiles=tuple(a.percentiles), credible=a.credible, doi=a.doi,
                           classes=classes, intervals=a.intervals, mixtures=a.mixtures)
        dst = save(out, output_path(f))
        print("%s -> %s (%d soundings)" % (f, dst, out["mean"].shape[0]))
        if a.elevation_axis is not None:
            from . import elevation, hdf
            arrays, _ = hdf.load_results(f)
            surface = _key(arrays, "/data/elevation/data", "/data/elevation")
            if surface is None or np.asarray(surface).size != out["mean"].shape[0]:
                print("%s holds no /data/elevation to hang an elevation axis on" % f, file=sys.stderr)
                return 1
            dz, top, bottom = elevation_axis_arguments(a.elevation_axis)
            try:
                edges = elevation.regular_axis(surface, out["depth_edges"], dz, top=top, bottom=bottom)
                dst = save(on_elevation(out, surface, edges=edges, device=a.device), elevation_output_path(f))
            except ValueError as e:
                print("line_products: %s: %s" % (f, e), file=sys.stderr)
                return 1
            print("%s -> %s (%d elevation cells of %g m, %g .. %g m)" % (f, dst, edges.size - 1, dz, edges[0], edges[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
