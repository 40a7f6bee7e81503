"""Elevation slices: per-sounding columns on the depth-below-surface axis resampled onto a shared ELEVATION axis, on the device
(csrc/gbp_elev.h) -- the reference's ``Inference2D.elevationSlice(elevation, values)`` (inversion/Inference2D.py:881-922) for every
sounding and every elevation at once.  The line products and ``survey_volume`` end on depth cells draped under the terrain; over relief
"depth cell 37" is another horizon at every sounding.  This is the step from there to horizontal slices, sections against elevation and
voxel volumes with a regular z axis: ``[N, n_depth]`` in, ``[N, n_elev]`` out, the ``[N, C]`` layout ``gridding.SibsonPlan.apply`` takes.

With ``e`` the depth edges, ``z_s`` a sounding's surface elevation and cell(d) = clip(searchsorted(e, d, side='right') - 1, 0, n - 1):

  level E            d = z_s - E; the value of cell(d) when e[0] < d < e[n] (both strict: a level on the surface itself is outside), else
                     NaN;
  interval (lo, hi)  d0 = z_s - lo, d1 = z_s - hi; the mean of the cells cell(d1) .. cell(d0) when d1 < e[n] and d0 > e[0], else NaN.

The reference's quirks are kept, because its numbers are what the tests pin.  An interval only has to OVERLAP the mesh: one that sticks
out above the surface or below the last edge averages the cells it still overlaps.  The mean weighs every cell alike, whatever part of
it the interval covers and however thick it is.  A NaN surface elevation gives NaN (every comparison is false) and NaN values propagate.
The mean is sum / count and the sum runs in the order of numpy's pairwise summation, which is what the reference's ``mean`` adds up: a
left-to-right sum differs from it in the last bits of about a fifth of the outputs.  There is no host fallback: ``resample`` refuses
tensors that are not on the device (a plain numpy statement of the rule lives in tests/elevation_reference.py).
"""
import numpy as np
import torch

from . import _lib
from ._args import host

LEVELS, INTERVALS = 0, 1            # GBP_ELEVATION_LEVELS / GBP_ELEVATION_INTERVALS
MAX_DEPTH_CELLS = 8191


def check_depth_edges(depth_edges):
    """The depth edges as a float64 array: at least two, finite, strictly increasing, at most 8191 cells."""
    e = np.asarray(host(depth_edges), dtype=np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0.0):
        raise ValueError("depth_edges: at least two finite, strictly increasing edges are needed")
    if e.size - 1 > MAX_DEPTH_CELLS:
        raise ValueError("depth_edges: at most %d depth cells, got %d" % (MAX_DEPTH_CELLS, e.size - 1))
    return e


def check_axis(levels=None, edges=None):
    """(mode, axis as a float64 array, E) of exactly one of ``levels`` (finite, any order, at least one) and ``edges`` (finite, strictly
    increasing, at least two: cell k is (edges[k], edges[k + 1]))."""
    if (levels is None) == (edges is None):
        raise ValueError("exactly one of levels and edges must be given")
    if levels is not None:
        a = np.asarray(host(levels), dtype=np.float64).reshape(-1)
        if a.size < 1 or not np.all(np.isfinite(a)):
            raise ValueError("levels: at least one elevation, all finite")
        return LEVELS, a, a.size
    a = np.asarray(host(edges), dtype=np.float64).reshape(-1)
    if a.size < 2 or not np.all(np.isfinite(a)) or not np.all(np.diff(a) > 0.0):
        raise ValueError("edges: at least two finite, strictly increasing elevation edges are needed")
    return INTERVALS, a, a.size - 1


def regular_axis(surface, depth_edges, dz, top=None, bottom=None):
    """Ascending elevation edges ``dz`` apart: multiples of ``dz`` from ``bottom`` (default: the lowest surface minus
    ``depth_edges[-1]``) snapped down to ``top`` (default: the highest surface) snapped up, so that by default every depth cell of every
    sounding falls inside the axis.  NaN surface elevations are ignored."""
    dz = float(dz)
    if not (dz > 0.0 and np.isfinite(dz)):
        raise ValueError("dz must be positive and finite")
    if top is None or bottom is None:
        s = np.asarray(host(surface), dtype=np.float64).reshape(-1)
        s = s[np.isfinite(s)]
        if s.size == 0:
            raise ValueError("no finite surface elevation to span an axis over")
        e = check_depth_edges(depth_edges)
    top = float(s.max()) if top is None else float(top)
    bottom = float(s.min() - e[-1]) if bottom is None else float(bottom)
    if not (np.isfinite(top) and np.isfinite(bottom) and bottom < top):
        raise ValueError("the axis needs finite bottom < top, got %g and %g" % (bottom, top))
    k0, k1 = int(np.floor(bottom / dz)), int(np.ceil(top / dz))
    if k1 - k0 > 1 << 24:
        raise ValueError("dz = %g gives %d cells between %g and %g" % (dz, k1 - k0, bottom, top))
    return np.arange(k0, k1 + 1, dtype=np.float64) * dz


def resample(values, surface, depth_edges, levels=None, edges=None, columns=None):
    """``values`` [N, n_depth] or [N, K, n_depth] on the device -> [N, E] or [N, K, E] float64 on the elevation axis.

    ``surface`` [N]: the soundings' surface elevation (a host array, or a float64 tensor on the values' device); ``depth_edges``
    [n_depth + 1]: the shared depth edges, increasing, uniform or not.  Exactly one of ``levels`` [E] (the value of the cell holding each
    level) and ``edges`` [E + 1] (ascending; the mean over each cell (edges[k], edges[k + 1])).  ``columns`` = (c0, c1) computes the
    columns c0 <= k < c1 of the axis only and returns [N, c1 - c0] / [N, K, c1 - c0].  float64 values; integer values (class indices
    such as ``highest_marginal``) are taken at levels only and come back as float64, NaN outside the mesh -- the mean of class indices
    means nothing, so intervals refuse them."""
    if not torch.is_tensor(values):
        raise _lib.NativeLibraryError("elevation.resample runs on the device (gbp_elevation_resample); there is no host fallback")
    mode, axis, E = check_axis(levels, edges)
    integer = not values.dtype.is_floating_point and not values.dtype.is_complex
    if integer and mode == INTERVALS:
        raise ValueError("integer values (class indices) cannot be averaged over elevation intervals: the mean of class indices means "
                         "nothing; slice them at levels")
    if not integer and values.dtype != torch.float64:
        raise ValueError("values must be float64 (or integer, at levels), got %s" % values.dtype)
    if values.dim() not in (2, 3) or values.shape[0] < 1 or values.shape[-1] < 1 or (values.dim() == 3 and values.shape[1] < 1):
        raise ValueError("values must be [N, n_depth] or [N, K, n_depth], nothing empty, got %r" % (tuple(values.shape),))
    e = check_depth_edges(depth_edges)
    N, n = values.shape[0], values.shape[-1]
    K = values.shape[1] if values.dim() == 3 else 1
    if e.size != n + 1:
        raise ValueError("depth_edges holds %d edges for %d depth cells" % (e.size, n))
    c0, c1 = (0, E) if columns is None else (int(columns[0]), int(columns[1]))
    if not 0 <= c0 < c1 <= E:
        raise ValueError("columns must be a window 0 <= c0 < c1 <= %d, got (%d, %d)" % (E, c0, c1))
    dev = values.device
    if dev.type != "cuda":
        raise _lib.NativeLibraryError("elevation.resample runs on the device (gbp_elevation_resample); there is no host fallback")
    if torch.is_tensor(surface) and surface.device == dev and surface.dtype == torch.float64:
        s = surface.reshape(-1).contiguous()
    else:
        s = torch.as_tensor(np.ascontiguousarray(host(surface), dtype=np.float64).reshape(-1)).to(dev)
    if s.numel() != N:
        raise ValueError("surface holds %d elevations for %d soundings" % (s.numel(), N))
    v = values.to(torch.float64).contiguous()
    out = torch.empty((N * K, c1 - c0), dtype=torch.float64, device=dev)
    te, ta = torch.as_tensor(e).to(dev), torch.as_tensor(axis).to(dev)
    _lib.call("gbp_elevation_resample", dev, mode, N * K, K, n, v, s, te, E, ta, c0, c1, out)
    return out.reshape(N, K, c1 - c0) if values.dim() == 3 else out
