"""What leaves the device of a block's conductivity-depth hit maps (csrc/gbp_hitmap.h): per-depth statistics for the survey summary and
the maps in run-length form for the results containers -- one streaming kernel each instead of transposes, cumulative sums and a
``nonzero`` over 9e8 cells.  The statistics are the reference's ``Histogram.mean`` / ``Histogram.percentile`` along the value axis of
the conductivity-depth posterior (statistics/Histogram.py:262-284, 369-401 -> mesh/Mesh.py:80-113, 173-215), in log10: pinned to values
the imported reference computed (tests/golden/make_hitmap_stats.py -> hitmap_stats.npz, tests/test_hitmap_gpu.py).  There is no
fallback: the entries refuse tensors that are not on the device (the torch formulations the kernels were first held to live in
tests/hitmap_reference.py)."""
import ctypes

import torch

from . import _lib
from .line_products import entropy_bits, log10_shift, quantiles, value_centres


def _entry(hm, name):
    """The name of the C entry: ``name`` for int32 maps, ``name``_i64 for int64 ones; other count types are refused."""
    if hm.dtype == torch.int32:
        return name
    if hm.dtype == torch.int64:
        return name + "_i64"
    raise TypeError("hit maps are int32 (or int64 interval marginals), not %s" % hm.dtype)


def statistics(hitmap, log_mean_prior, half_width):
    """Mean and 5 / 50 / 95 % points of log10 conductivity per depth cell from the hit maps [B, n_value, n_depth] (value-major, depth
    fastest) in one kernel (gbp_hitmap_statistics): sum(count x cell centre) / total + the prior mean, and the centre of the first cell
    whose cumulative share reaches the percentile (an empty column: the prior mean / the last cell, as the reference's)."""
    if hitmap.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.statistics runs on the device (gbp_hitmap_statistics); there is no host fallback")
    B, nv, nz = hitmap.shape
    hm = hitmap.contiguous()
    assert hm.dtype == torch.int32
    lmp = log_mean_prior.to(torch.float64).contiguous()
    out = torch.empty((4, B, nz), dtype=torch.float64, device=hm.device)
    _lib.call("gbp_hitmap_statistics", hm.device, B, nv, nz, hm, lmp, float(half_width), out[0], out[1], out[2], out[3])
    return out[0], [out[1], out[2], out[3]]


def runs(hitmap):
    """(ptr int64 [B + 1], start int32, value) of the rows of ``hitmap`` flattened -- a run starts at cell 0 and at every change of
    value -- as two passes of one kernel (gbp_hitmap_runs: count, prefix, write)."""
    if hitmap.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.runs runs on the device (gbp_hitmap_runs); there is no host fallback")
    hm = hitmap.flatten(1).contiguous()
    assert hm.dtype == torch.int32
    B, M = hm.shape
    dev = hm.device
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    if B == 0:
        return ptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    _lib.call("gbp_hitmap_runs", dev, B, M, hm, ptr[1:], None, None, None)
    torch.cumsum(ptr[1:], 0, out=ptr[1:])
    n = int(ptr[-1])
    start = torch.empty(n, dtype=torch.int32, device=dev)
    value = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("gbp_hitmap_runs", dev, B, M, hm, None, ptr, start, value)
    return ptr, start, value


def moments(hitmap, log_mean_prior, half_width, q):
    """The per-column moments of the hit maps [B, n_value, n_depth] in one kernel (gbp_hitmap_products): mean (log10, the bits of
    ``statistics``), mode_idx, q_idx [len(q), B, n_depth], total (int64) and s1 = sum c ln c, on the maps' device.  int32 maps, or
    int64 ones (``interval_marginals``: gbp_hitmap_products_i64, the same kernel on the other count type)."""
    if hitmap.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.moments runs on the device (gbp_hitmap_products); there is no host fallback")
    B, nv, nz = hitmap.shape
    hm = hitmap.contiguous()
    entry = _entry(hm, "gbp_hitmap_products")
    dev = hm.device
    lmp = log_mean_prior.to(device=dev, dtype=torch.float64).contiguous()
    qa = (ctypes.c_double * max(len(q), 1))(*q)
    mean = torch.empty((B, nz), dtype=torch.float64, device=dev)
    s1 = torch.empty((B, nz), dtype=torch.float64, device=dev)
    total = torch.empty((B, nz), dtype=torch.int64, device=dev)
    mode_idx = torch.empty((B, nz), dtype=torch.int32, device=dev)
    q_idx = torch.empty((len(q), B, nz), dtype=torch.int32, device=dev)
    _lib.call(entry, dev, B, nv, nz, hm, lmp, float(half_width), len(q), qa, mean, mode_idx, q_idx, total, s1)
    return dict(mean=mean, mode_idx=mode_idx, q_idx=q_idx, total=total, s1=s1)


def products(hitmap, log_mean_prior, half_width, percentiles=(5, 50, 95), credible=90.0, depth_edges=None):
    """Per-sounding posterior products of the hit maps [B, n_value, n_depth] in log10 conductivity, each [B, n_depth] on the maps' device
    (the reference's ``Histogram`` along the value axis, statistics/Histogram.py): ``mean``, ``median``, ``mode`` (the centre of the first
    cell of the largest count), ``percentile_<p>`` for each requested p, ``credible_low`` / ``credible_high`` / ``credible_range`` of the
    ``credible`` % interval (``credible_range(credible, log=10)``), and ``entropy`` in bits (``Histogram.entropy``: the sum over the value
    cells of -p log2 p with p the DENSITY c / sum(area c) over the sounding's cells of area dvalue x ddepth; ``depth_edges`` gives ddepth,
    unit depth cells when None).  One kernel pass (``moments``) and elementwise finishing (line_products)."""
    B, nv, nz = hitmap.shape
    q, pos, (klo, khi) = quantiles(percentiles, credible)
    m = moments(hitmap, log_mean_prior, half_width, q)
    dev = m["mean"].device
    shift = log10_shift(log_mean_prior).to(dev)[:, None]
    centre = lambda idx: value_centres(idx, nv, half_width, shift)          # noqa: E731
    out = dict(mean=m["mean"], median=centre(m["q_idx"][pos[50.0]]), mode=centre(m["mode_idx"]))
    for p in percentiles:
        out["percentile_%g" % float(p)] = centre(m["q_idx"][pos[float(p)]])
    out["credible_low"], out["credible_high"] = centre(m["q_idx"][klo]), centre(m["q_idx"][khi])
    out["credible_range"] = (out["credible_high"] - out["credible_low"]).abs()
    dz = torch.ones(nz, dtype=torch.float64, device=dev) if depth_edges is None else \
        torch.diff(torch.as_tensor(depth_edges, dtype=torch.float64, device=dev)).abs()
    out["entropy"] = entropy_bits(m["total"], m["s1"], dz * (2.0 * float(half_width) / nv))
    out["total"], out["s1"] = m["total"], m["s1"]
    return out


def class_probability(hitmap, log_mean_prior, half_width, means, scales):
    """Class (lithology) probabilities of the hit maps [B, n_value, n_depth] in one kernel (gbp_hitmap_classes), on the maps' device: K
    classes in log10 conductivity (S/m), class k weighting value cell v by norm.pdf(x_v, means[k], scales[k]) at the cell's centre x_v
    (the centres of ``statistics``), normalised over the classes per depth cell -- the reference's ``compute_probability(MvNormal(means,
    variance), log=10, axis=0)`` (mesh/RectilinearMesh2D.py _compute_probability), whose "variance" reaches scipy as the scale: here
    ``scales`` are standard deviations.  Every class has the same prior weight.  Returns ``probability`` [B, K, n_depth] (NaN where every
    term is 0, e.g. an empty column), ``highest_marginal`` [B, n_depth] int32 (the first most probable class; numpy's argmax over the
    class axis, 0 for a NaN column) and ``probability_of_highest_marginal`` [B, n_depth] (its probability, NaN for a NaN column).
    1 <= K <= 16, and K n_value fp64 weights must fit in 64 KiB (gbp_hitmap_classes refuses the rest).  int32 maps, or int64 ones
    (``interval_marginals``: gbp_hitmap_classes_i64)."""
    if hitmap.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.class_probability runs on the device (gbp_hitmap_classes); there is no host fallback")
    B, nv, nz = hitmap.shape
    hm = hitmap.contiguous()
    entry = _entry(hm, "gbp_hitmap_classes")
    dev = hm.device
    mu = [float(m) for m in means]
    sd = [float(s) for s in scales]
    if len(mu) != len(sd):
        raise ValueError("class_probability: %d means but %d scales" % (len(mu), len(sd)))
    K = len(mu)
    lmp = log_mean_prior.to(device=dev, dtype=torch.float64).contiguous()
    ma = (ctypes.c_double * max(K, 1))(*mu)
    sa = (ctypes.c_double * max(K, 1))(*sd)
    prob = torch.empty((B, K, nz), dtype=torch.float64, device=dev)
    best = torch.empty((B, nz), dtype=torch.int32, device=dev)
    best_p = torch.empty((B, nz), dtype=torch.float64, device=dev)
    _lib.call(entry, dev, B, nv, nz, hm, lmp, float(half_width), K, ma, sa, prob, best, best_p)
    return dict(probability=prob, highest_marginal=best, probability_of_highest_marginal=best_p)


def interval_marginals(hitmap, lo, hi):
    """Interval marginals of the hit maps [B, n_value, n_depth] (int32) in one kernel (gbp_hitmap_intervals), on the maps' device:
    int64 [B, n_value, M], the counts summed over the depth cells ``lo <= cell < hi`` of each of M ranges (``intervals.depth_ranges``
    and its siblings) -- the reference's ``Histogram[:, lo:hi].marginalize(axis=1)``.  ``lo`` / ``hi``: [M] (every sounding the same)
    or [B, M], integers; clamped to [0, n_depth] by the kernel, ``hi <= lo``: no cells, zeros.  Ranges may overlap.  int64 because a few
    cells of a long chain's map sum beyond 2^31.  ``products`` / ``class_probability`` take the result as they take the maps."""
    if hitmap.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.interval_marginals runs on the device (gbp_hitmap_intervals); there is no host fallback")
    B, nv, nz = hitmap.shape
    hm = hitmap.contiguous()
    if hm.dtype != torch.int32:
        raise TypeError("hit maps are int32, not %s" % hm.dtype)
    dev = hm.device

    def ranges(r):
        r = torch.as_tensor(r)
        if r.dtype.is_floating_point or r.dtype == torch.bool or r.ndim not in (1, 2):
            raise ValueError("interval ranges are integers [M] or [B, M]")
        r = r.clamp(-1, nz + 1).to(device=dev, dtype=torch.int32)
        if r.ndim == 1:
            r = r[None, :].expand(B, -1)
        if r.shape[0] != B:
            raise ValueError("interval ranges for %d soundings, the block has %d" % (r.shape[0], B))
        return r.contiguous()

    lo_d, hi_d = ranges(lo), ranges(hi)
    if lo_d.shape != hi_d.shape:
        raise ValueError("lo and hi differ in shape: %r, %r" % (tuple(lo_d.shape), tuple(hi_d.shape)))
    M = lo_d.shape[1]
    out = torch.empty((B, nv, M), dtype=torch.int64, device=dev)
    _lib.call("gbp_hitmap_intervals", dev, B, nv, nz, M, hm, lo_d, hi_d, out)
    return out


def _mixture_arguments(maps, half_width, max_components, n_iter, reg):
    """The checks of ``mixture`` that need no device: (Kmax, n_iter, reg), with the default reg = dx^2 / 12."""
    if not isinstance(maps, torch.Tensor) or maps.ndim != 3:
        raise TypeError("hit maps are a tensor [B, n_value, n_depth]")
    if maps.dtype not in (torch.int32, torch.int64):
        raise TypeError("hit maps are int32 (or int64 interval marginals), not %s" % maps.dtype)
    if not maps.is_contiguous():
        raise ValueError("hit maps must be contiguous (depth fastest)")
    if maps.shape[1] < 1 or maps.shape[2] < 1:
        raise ValueError("hit maps need at least one value cell and one depth cell, got %r" % (tuple(maps.shape),))
    from . import mixtures
    return mixtures.check_arguments(maps.shape[1], half_width, max_components, n_iter, reg)


def mixture(maps, half_width, max_components=3, n_iter=50, reg=None):
    """Local mixture fits in one kernel (gbp_hitmap_mixture): every stage K = 1 .. ``max_components`` (at most 4) of the
    rule of ``mixtures.mixture_reference`` for every column of ``maps`` [B, n_value, n_depth] (int32, or int64 interval marginals:
    gbp_hitmap_mixture_i64), K Gaussians fitted to the binned column by ``n_iter`` EM iterations from the quantile start; ``reg`` is
    added to every variance (default dx^2 / 12, a value cell's own variance).  Returns the stages on the maps' device: ``weight`` /
    ``mean`` / ``sd`` [B, Kmax (Kmax + 1) / 2, n_depth] (stage K in slots K (K - 1) / 2 .. + K; means WITHOUT the prior shift), ``loglik``
    / ``ll_change`` [B, Kmax, n_depth] and ``misfit`` [B, Kmax, 2, n_depth] (the relative max and 2-norms of pmf minus fit); NaN for an
    empty column.  ``mixtures.select`` picks a stage per column."""
    K, n, reg = _mixture_arguments(maps, half_width, max_components, n_iter, reg)
    if maps.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.mixture runs on the device (gbp_hitmap_mixture); there is no host fallback")
    entry = _entry(maps, "gbp_hitmap_mixture")
    B, nv, nz = maps.shape
    dev = maps.device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    S = K * (K + 1) // 2
    out = dict(weight=f64(B, S, nz), mean=f64(B, S, nz), sd=f64(B, S, nz), loglik=f64(B, K, nz), ll_change=f64(B, K, nz),
               misfit=f64(B, K, 2, nz))
    _lib.call(entry, dev, B, nv, nz, maps, float(half_width), K, n, reg, out["weight"], out["mean"], out["sd"], out["loglik"], out["ll_change"],
              out["misfit"])
    return out


def _pool_arguments(maps, C, use, max_total=None):
    """The checks of ``pool`` that need no device: (S, C, use as int32 [S, C] on the maps' device)."""
    if not isinstance(maps, torch.Tensor) or maps.ndim != 3:
        raise TypeError("replicate hit maps are a tensor [S * C, n_value, n_depth]")
    if maps.dtype != torch.int32:
        raise TypeError("hit maps are int32, not %s" % maps.dtype)
    if not maps.is_contiguous():
        raise ValueError("replicate hit maps must be contiguous (depth fastest)")
    C = int(C)
    if not 2 <= C <= 8:
        raise ValueError("pool: C = %d replicate chains, 2 .. 8 are supported" % C)
    if maps.shape[0] % C:
        raise ValueError("pool: %d maps are not %d chains per sounding" % (maps.shape[0], C))
    S = maps.shape[0] // C
    if use is None:
        use = torch.ones((S, C), dtype=torch.int32, device=maps.device)
    else:
        use = torch.as_tensor(use)
        if tuple(use.shape) != (S, C):
            raise ValueError("pool: use must be [%d, %d], not %r" % (S, C, tuple(use.shape)))
        use = (use != 0).to(device=maps.device, dtype=torch.int32).contiguous()
    # a pooled cell is at most C times the largest column total (a column's total is at most the chain's sample count); without a
    # bound from the caller the totals are formed here: one more read of the maps and a host synchronisation
    if max_total is None:
        max_total = int(maps.sum(dim=1, dtype=torch.int64).max()) if maps.numel() else 0
    if C * int(max_total) > 0x7fffffff:
        raise ValueError("pool: %d chains of up to %d samples per column could pass 2^31 - 1 in a pooled int32 cell" % (C, int(max_total)))
    return S, C, use


def pool(maps, C, use=None, half_width=1.0, max_total=None):
    """Replicate chains in one kernel (gbp_hitmap_pool): ``maps`` int32 [S * C, n_value, n_depth], row s * C + c the
    replicate c of sounding s; ``use`` [S, C] (non-zero: the chain takes part; None: all).  Returns ``pooled`` int32 [S, n_value,
    n_depth] (the sum over the used chains), ``n_used`` int32 [S, n_depth] (used chains with samples in the column), ``chain_mean``
    [S, C, n_depth] (the chains' column means on the value axis WITHOUT the prior shift, NaN for a chain that takes no part), ``rhat``
    [S, n_depth] (Gelman-Rubin potential scale reduction of the column means) and ``jsd`` [S, n_depth] (generalised Jensen-Shannon
    divergence of the chains' columns, bits: 0 identical, log2 n_used disjoint); both NaN with fewer than two chains.  The axis is
    generic: a histogram [S * C, cells] is ``maps[:, :, None]``.  A block whose pooled int32 cells could overflow is refused: C times
    ``max_total``, an upper bound of every column's total that the caller knows (a chain's sample count), else the largest column
    total, found by one more read of the maps.  The host statement of the rule is ``replicates.pool_reference``."""
    S, C, use = _pool_arguments(maps, C, use, max_total)
    if maps.device.type != "cuda":
        raise _lib.NativeLibraryError("hitmap.pool runs on the device (gbp_hitmap_pool); there is no host fallback")
    _, nv, nz = maps.shape
    dev = maps.device
    out = dict(pooled=torch.empty((S, nv, nz), dtype=torch.int32, device=dev), n_used=torch.empty((S, nz), dtype=torch.int32, device=dev),
               chain_mean=torch.empty((S, C, nz), dtype=torch.float64, device=dev), rhat=torch.empty((S, nz), dtype=torch.float64, device=dev),
               jsd=torch.empty((S, nz), dtype=torch.float64, device=dev))
    _lib.call("gbp_hitmap_pool", dev, S, C, nv, nz, maps, use, float(half_width), out["pooled"], out["n_used"], out["chain_mean"], out["rhat"],
              out["jsd"])
    return out
