"""Depth-cell ranges of units: which cells of a sounding's depth mesh make up "the top 10 m", "30 - 75 m", "between -40 and -10 m
elevation" or "between the top and the base of a picked horizon".  The ranges feed ``hitmap.interval_marginals`` (csrc/gbp_hitmap.h
k_hitmap_intervals), which sums the hit map's counts over each range -- the unit's marginal posterior, the reference's
``Histogram[:, lo:hi].marginalize(axis=1)`` (statistics/Histogram.py:60-64, 236-260) -- and the statistics of ``hitmap.products`` /
``hitmap.class_probability`` then run along the value axis of those marginals (``line_products.from_results(intervals=...)``).

A range is half-open, ``lo <= cell < hi``; whole cells only, assigned by their CENTRES 0.5 (e[1:] + e[:-1]), the rule of the reference's
``RectilinearMesh2D.intervalStatistic`` (mesh/RectilinearMesh2D.py:507-558), which bins the cell centres with
``scipy.stats.binned_statistic``: cell z belongs to interval m when edges[m] <= centre_z < edges[m + 1], and the LAST interval also takes
centre_z == edges[-1].  A pair of depths follows ``Inference2D._z_slice`` instead (``survey_volume.depth_cells``): the cells holding both
depths and those between.  Ranges only partly inside the mesh take the cells they have, ranges outside it have none (``n_cells`` 0).

Everything here is host numpy on small [N, M] arrays; one fp64 subtraction (surface - centre) puts a cell on the elevation axis.
"""
import collections

import numpy as np

Ranges = collections.namedtuple("Ranges", "lo hi n_cells")     # int32 arrays, [M] or [N, M]; n_cells = hi - lo

KINDS = ("depth", "pairs", "elevation", "horizons")


def depth_centres(depth_edges):
    """Centres of the depth cells, 0.5 (e[1:] + e[:-1]) (the bits of the reference's ``mesh.y.centres``), of ascending edges."""
    e = np.asarray(depth_edges, dtype=np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0.0):
        raise ValueError("depth_edges must be finite and ascending, at least two")
    return 0.5 * (e[1:] + e[:-1])


def _ascending(edges, what):
    x = np.asarray(edges, dtype=np.float64).reshape(-1)
    if x.size < 2 or not np.all(np.isfinite(x)) or not np.all(np.diff(x) > 0.0):
        raise ValueError("%s must be at least two finite ascending edges" % what)
    return x


def _ranges(lo, hi):
    lo = np.asarray(lo, dtype=np.int64)
    hi = np.maximum(np.asarray(hi, dtype=np.int64), lo)
    return Ranges(lo.astype(np.int32), hi.astype(np.int32), (hi - lo).astype(np.int32))


def depth_ranges(depth_edges, edges):
    """Ranges [M] of the M intervals between the ascending ``edges`` [M + 1] (m below the surface): the centre rule."""
    c = depth_centres(depth_edges)
    x = _ascending(edges, "interval edges")
    below = np.searchsorted(c, x, side="left")                 # cells whose centre lies below each edge
    hi = below[1:].copy()
    hi[-1] = np.searchsorted(c, x[-1], side="right")           # the closed last edge
    return _ranges(below[:-1], hi)


def depth_pairs(depth_edges, pairs):
    """Ranges [M] of M pairs of depths (floats, m) or of cells (ints; inclusive): ``survey_volume.depth_cells``'s rule for a pair --
    the cells holding both depths and those between.  Pairs may overlap; a pair reaching beyond the mesh takes the cells inside it."""
    from .survey_volume import depth_cells
    e = np.asarray(depth_edges, dtype=np.float64).reshape(-1)
    depth_centres(e)
    nz = e.size - 1
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("pairs must be [M, 2]")
    lo, hi = [], []
    for a, b in p:
        if p.dtype.kind in "iu":
            a, b = sorted((int(a), int(b)))
            a, b = max(a, 0), min(b, nz - 1)
            s = depth_cells((a, b), e) if a <= b else slice(0, 0)
        else:
            a, b = sorted((float(a), float(b)))
            if not (np.isfinite(a) and np.isfinite(b)) or b < e[0] or a >= e[-1]:
                s = slice(0, 0)
            else:
                s = depth_cells((max(a, e[0]), b if b < e[-1] else 0.5 * (e[-2] + e[-1])), e)
        lo.append(s.start)
        hi.append(s.stop)
    return _ranges(lo, hi)


def _below_surface(surface, depth_edges):
    """-(surface - centre) [N, n_depth]: ascending along depth, the negated elevation of every cell centre."""
    s = np.asarray(surface, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(s)):
        raise ValueError("the surface elevations must be finite")
    return -(s[:, None] - depth_centres(depth_edges)[None, :])


def elevation_ranges(surface, depth_edges, edges):
    """Ranges [N, M] of the M elevation intervals between the ascending ``edges`` [M + 1] (m; interval 0 the lowest) under each
    sounding's ``surface`` [N]: the centre rule on surface - centre, edges[m] <= surface - centre_z < edges[m + 1], the last interval
    closed above."""
    neg = _below_surface(surface, depth_edges)
    x = _ascending(edges, "interval edges")
    at_or_above = np.stack([(neg <= -v).sum(axis=1) for v in x], axis=1)      # [N, M + 1]: cells with elevation >= each edge
    lo = at_or_above[:, 1:].copy()                                             # (those at or above the upper edge are out)
    lo[:, -1] = (neg < -x[-1]).sum(axis=1)                                     # the closed last edge
    return _ranges(lo, at_or_above[:, :-1])


def horizon_ranges(depth_edges, top, bottom, surface=None):
    """Ranges [N, M] of the units between the horizons ``top`` and ``bottom`` ([N] or [N, M]): depths below the surface (m), or
    elevations when ``surface`` [N] is given.  The cells with top <= centre < bottom in depth terms (with a surface:
    bottom < surface - centre <= top).  A NaN bound, or a bottom not below its top, gives no cells."""
    t = np.asarray(top, dtype=np.float64)
    b = np.asarray(bottom, dtype=np.float64)
    if t.shape != b.shape or t.ndim not in (1, 2):
        raise ValueError("top and bottom must both be [N] or [N, M]")
    t, b = (t[:, None], b[:, None]) if t.ndim == 1 else (t, b)
    bad = np.isnan(t) | np.isnan(b)
    t0, b0 = np.where(bad, 0.0, t), np.where(bad, 0.0, b)
    if surface is None:
        c = depth_centres(depth_edges)
        lo, hi = np.searchsorted(c, t0, side="left"), np.searchsorted(c, b0, side="left")
    else:
        neg = _below_surface(surface, depth_edges)
        if neg.shape[0] != t.shape[0]:
            raise ValueError("%d surface elevations but %d soundings of horizons" % (neg.shape[0], t.shape[0]))
        lo = np.stack([(neg < -t0[:, m:m + 1]).sum(axis=1) for m in range(t.shape[1])], axis=1)    # cells above the top
        hi = np.stack([(neg < -b0[:, m:m + 1]).sum(axis=1) for m in range(t.shape[1])], axis=1)    # cells above the bottom
    hi = np.where(bad, lo, hi)
    return _ranges(lo, hi)


def check_spec(spec):
    """``spec`` (a dict, or an object with the same attributes) as a dict with ``kind`` in depth / pairs / elevation / horizons and
    its arrays as numpy: ``edges`` (depth, elevation), ``pairs`` (pairs), ``top`` / ``bottom`` (horizons), and optionally ``surface``
    [N] (elevation: default the container's /data/elevation; horizons: given -> the horizons are elevations, True -> elevations under
    the container's)."""
    d = dict(spec) if isinstance(spec, dict) else {k: getattr(spec, k) for k in ("kind", "edges", "pairs", "top", "bottom", "surface")
                                                   if getattr(spec, k, None) is not None}
    kind = d.get("kind")
    if kind not in KINDS:
        raise ValueError("intervals: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    out = dict(kind=kind)
    allowed = {"depth": ("edges",), "pairs": ("pairs",), "elevation": ("edges", "surface"), "horizons": ("top", "bottom", "surface")}[kind]
    extra = set(d) - set(allowed) - {"kind"}
    if extra:
        raise ValueError("intervals: a %s spec takes %s, not %s" % (kind, ", ".join(allowed), ", ".join(sorted(extra))))
    if kind in ("depth", "elevation"):
        out["edges"] = _ascending(d.get("edges", ()), "intervals: edges")
    elif kind == "pairs":
        p = np.asarray(d.get("pairs", ()))
        if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.dtype.kind not in "iuf":
            raise ValueError("intervals: pairs must be [M, 2] depths or cells")
        out["pairs"] = p if p.dtype.kind in "iu" else p.astype(np.float64)
    else:
        if "top" not in d or "bottom" not in d:
            raise ValueError("intervals: horizons need top and bottom")
        out["top"], out["bottom"] = np.asarray(d["top"], dtype=np.float64), np.asarray(d["bottom"], dtype=np.float64)
    if d.get("surface") is not None:
        out["surface"] = True if d["surface"] is True else np.asarray(d["surface"], dtype=np.float64).reshape(-1)
    return out


def n_intervals(spec):
    """M of a checked spec."""
    if spec["kind"] in ("depth", "elevation"):
        return spec["edges"].size - 1
    if spec["kind"] == "pairs":
        return spec["pairs"].shape[0]
    return 1 if spec["top"].ndim == 1 else spec["top"].shape[1]


def ranges(spec, depth_edges, n_soundings, surface=None):
    """Ranges [N, M] of a checked ``spec`` for a line of ``n_soundings`` over ``depth_edges``; ``surface`` [N]: the line's own surface
    elevations, used where the spec needs them and brings none."""
    kind = spec["kind"]
    N = int(n_soundings)
    own = spec.get("surface")
    if kind == "elevation" or (kind == "horizons" and own is not None):
        s = surface if (own is None or own is True) else own
        if s is None or np.asarray(s).size != N:
            raise ValueError("intervals: %s ranges need %d surface elevations" % (kind, N))
    if kind == "depth":
        r = depth_ranges(depth_edges, spec["edges"])
    elif kind == "pairs":
        r = depth_pairs(depth_edges, spec["pairs"])
    elif kind == "elevation":
        return elevation_ranges(s, depth_edges, spec["edges"])
    else:
        if spec["top"].shape[0] != N:
            raise ValueError("intervals: horizons for %d soundings, the line has %d" % (spec["top"].shape[0], N))
        return horizon_ranges(depth_edges, spec["top"], spec["bottom"], surface=None if own is None else s)
    return Ranges(*(np.broadcast_to(a, (N, a.size)).copy() for a in r))


def unit_bounds(spec, n_soundings, surface=None, max_depth=None):
    """Exact bounds [N, M, 2] (top, bottom; m below the surface) of the units of a ``spec`` -- what the SAMPLED unit posteriors
    integrate over (``rjmcmc_gpu.DeviceChains(units=...)``, ``inference.Posteriors(units=...)``), where ``ranges`` gives whole cells of
    the depth mesh.  ``depth``: the intervals between the edges; ``elevation``: between the edges under each sounding's ``surface`` [N],
    lowest unit first as ``elevation_ranges`` orders them; ``horizons``: top / bottom as depths, or as elevations when the spec asks for
    a surface; ``pairs`` of depths (floats).  Bounds are clipped to [0, ``max_depth``] (no ``max_depth``: to [0, inf) -- give one, the
    sampler wants finite bounds); a unit wholly above the ground or below ``max_depth``, a NaN horizon or a bottom not below its top
    gives top == bottom: the unit has no posterior."""
    spec = check_spec(spec)
    kind, N = spec["kind"], int(n_soundings)
    own = spec.get("surface")
    s = None
    if kind == "elevation" or (kind == "horizons" and own is not None):
        s = surface if (own is None or own is True) else own
        if s is None or np.asarray(s).size != N:
            raise ValueError("intervals: %s units need %d surface elevations" % (kind, N))
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(s)):
            raise ValueError("the surface elevations must be finite")
    if kind == "depth":
        x = spec["edges"]
        z0, z1 = np.broadcast_to(x[:-1], (N, x.size - 1)), np.broadcast_to(x[1:], (N, x.size - 1))
    elif kind == "pairs":
        if spec["pairs"].dtype.kind != "f":
            raise ValueError("intervals: unit bounds need pairs of depths, not of cells")
        pr = np.sort(spec["pairs"], axis=1)
        z0, z1 = np.broadcast_to(pr[:, 0], (N, pr.shape[0])), np.broadcast_to(pr[:, 1], (N, pr.shape[0]))
    elif kind == "elevation":
        x = spec["edges"]
        z0, z1 = s[:, None] - x[None, 1:], s[:, None] - x[None, :-1]
    else:
        t, b = spec["top"], spec["bottom"]
        t, b = (t[:, None], b[:, None]) if t.ndim == 1 else (t, b)
        if t.shape[0] != N:
            raise ValueError("intervals: horizons for %d soundings, the line has %d" % (t.shape[0], N))
        z0, z1 = (t, b) if s is None else (s[:, None] - t, s[:, None] - b)
    top = None if max_depth is None else float(max_depth)
    z0, z1 = np.array(z0, dtype=np.float64), np.array(z1, dtype=np.float64)
    bad = ~(np.isfinite(z0) & np.isfinite(z1))
    z0, z1 = np.where(bad, 0.0, z0), np.where(bad, 0.0, z1)
    z0, z1 = np.clip(z0, 0.0, top), np.clip(z1, 0.0, top)
    return np.stack([z0, np.maximum(z1, z0)], axis=2)


def describe(spec):
    """The spec as ``interval_*`` entries of the products: ``interval_kind`` and its arrays."""
    out = {"interval_kind": np.array(spec["kind"])}
    for k in ("edges", "pairs", "top", "bottom"):
        if k in spec:
            out["interval_" + k] = spec[k]
    if isinstance(spec.get("surface"), np.ndarray):
        out["interval_surface"] = spec["surface"]
    elif spec.get("surface") is True:
        out["interval_surface_from_container"] = np.array(True)
    return out


def same_spec(products, spec):
    """Whether the saved ``products`` hold interval entries computed for exactly ``spec`` (checked)."""
    want = describe(spec)
    have = {k for k in products if k in ("interval_kind", "interval_edges", "interval_pairs", "interval_top", "interval_bottom",
                                          "interval_surface", "interval_surface_from_container")}
    if have != set(want):
        return False
    for k, v in want.items():
        a, b = np.asarray(products[k]), np.asarray(v)
        if a.shape != b.shape or a.dtype.kind != b.dtype.kind or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            return False
    return True


def edges_argument(values):
    """The edges of the command lines' ``--depth-intervals`` / ``--elevation-intervals E0 E1 ...``, checked: at least two, finite,
    ascending."""
    return _ascending([float(v) for v in values], "the edges")
