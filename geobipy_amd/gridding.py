"""Gridding of soundings onto a regular x-y raster by discrete Sibson (natural-neighbour) interpolation: the reference's
``method='sibson'`` (base/interpolation.py ``sibson`` -> ``__sibson_2d_inner``, reached from ``Point.interpolate`` and from there by
``Inference3D.interpolate_3d`` / ``map_depth_slice``), on the device (csrc/gbp_grid.h).

Every raster pixel (i, j) finds the sounding nearest to its lower-left NODE (j, i) in pixel coordinates, at distance r, and adds that
sounding's value to every pixel within D = ceil(r) of itself; a pixel's result is the average of what it received.  The reference's
quirks are kept, because its numbers are what the tests pin: the window of a pixel is i - D <= i_s < i + D (upper bound exclusive, so the
disc is lopsided and a pixel with D = 0 covers nothing, not even itself), the disc test is (i_s - i)^2 + (j_s - j)^2 <= D^2 + 0.25, a
pixel nobody covers is NaN (0 / 0), and ``max_distance`` masks the pixels whose own D^2 + 0.25 exceeds max_distance / (dx dy) -- pixels
squared against metres per metre squared, as the reference compares them -- while a masked pixel still covers its neighbours.

The reference repeats the whole sweep per depth cell and per variable.  The geometry does not depend on the values, so here it is a
``SibsonPlan`` (nearest sounding, D, and per destination pixel the list of covering pixels in row-major order), built once per grid,
and ``SibsonPlan.apply`` streams any number of columns ``[N, C]`` through it.  The sums run in the reference's order of additions (the
row-major order of the covering pixels), which makes the results equal to the reference's in every bit and reproducible from run to run;
the library uses no atomics and no partial sums for them.  There is no host fallback: the entries refuse tensors that are not on the
device (a plain numpy statement of the algorithm lives in tests/sibson_reference.py).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._args import host


def centred_grid_nodes(bounds, spacing):
    """Grid nodes centred over ``bounds`` = (min, max): arange(min - s / 2, max + s, s) (the reference's ``Point.centred_grid_nodes``)."""
    if not float(spacing) > 0.0:
        raise ValueError("spacing must be positive")
    sp = 0.5 * spacing
    return np.arange(bounds[0] - sp, bounds[1] + (2 * sp), spacing)


def centred_mesh(x, y, dx, dy):
    """(x_edges, y_edges) of the reference's ``Point.centred_mesh(dx, dy)`` over the soundings' bounding box (nanmin / nanmax)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return centred_grid_nodes((np.nanmin(x), np.nanmax(x)), dx), centred_grid_nodes((np.nanmin(y), np.nanmax(y)), dy)


def _uniform_edges(edges, name):
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)):
        raise ValueError("%s: at least two finite grid edges are needed" % name)
    step = e[1] - e[0]
    if not step > 0.0 or np.abs(np.diff(e) - step).max() > 1e-9 * step + 8.0 * np.spacing(np.abs(e).max()):
        raise ValueError("%s: the grid edges must be uniform and increasing (the Sibson raster has one pixel size per axis)" % name)
    return e, step


def pixel_coordinates(x, y, x_edges, y_edges):
    """(px, py, dx, dy): the soundings in units of pixels from the grid's first node, (x - x_edges[0]) / dx with dx = x_edges[1] -
    x_edges[0], computed by numpy as the reference does (base/interpolation.py:37-43; ``line_products.log10_shift`` records why the
    division is not left to torch on the device).  Non-uniform edges are refused."""
    xe, dx = _uniform_edges(x_edges, "x_edges")
    ye, dy = _uniform_edges(y_edges, "y_edges")
    x = np.array(x, dtype=np.float64).reshape(-1)
    y = np.array(y, dtype=np.float64).reshape(-1)
    if x.size != y.size or x.size < 1:
        raise ValueError("x and y must hold the same number of soundings, at least one (got %d and %d)" % (x.size, y.size))
    x -= xe[0]
    x = x / dx
    y -= ye[0]
    y = y / dy
    return x, y, dx, dy


def axis_offsets(log_mean_prior, half_width, n_value):
    """u [N] float64: the soundings' axis offsets in value cells, ``log10_shift(log_mean_prior) / w`` with w = 2 half_width / n_value,
    computed once by numpy on the host so that the device only subtracts and rounds."""
    from .line_products import log10_shift
    w = 2.0 * float(half_width) / int(n_value)
    return log10_shift(np.asarray(log_mean_prior, dtype=np.float64)).numpy() / w


def _pool_arguments(plan, maps, pixels, log_mean_prior, half_width, max_total, out=None):
    """The checks of ``SibsonPlan.pool`` that need no device: (pixels int64 [P], u float64 [N] or None, log_mean_prior float64 [N] or
    None), all on the host."""
    if not isinstance(maps, torch.Tensor) or maps.ndim != 3:
        raise TypeError("gbp_sibson_pool: hit maps are a tensor [N, n_value, n_depth]")
    if maps.dtype != torch.int32:
        raise TypeError("gbp_sibson_pool: hit maps are int32, not %s" % maps.dtype)
    if not maps.is_contiguous():
        raise ValueError("gbp_sibson_pool: hit maps must be contiguous (depth fastest)")
    N, nv, nz = maps.shape
    if N != plan.n_soundings or nv < 1 or nz < 1:
        raise ValueError("gbp_sibson_pool: maps of %d soundings with at least one value and one depth cell are needed, got %r" % (
            plan.n_soundings, tuple(maps.shape)))
    P = plan.nx * plan.ny
    if pixels is None:
        pix = np.arange(P, dtype=np.int64)
    else:
        pix = host(pixels)
        if pix.dtype.kind not in "iu" or pix.ndim != 1:
            raise TypeError("gbp_sibson_pool: pixels are a list [P] of integers (flat pixel numbers), got %s %r" % (pix.dtype, pix.shape))
        pix = pix.astype(np.int64)
        if pix.size and (pix.min() < 0 or pix.max() >= P):
            raise ValueError("gbp_sibson_pool: pixel %d is outside the raster of %d x %d pixels" % (
                pix[(pix < 0) | (pix >= P)][0], plan.ny, plan.nx))
    if (log_mean_prior is None) != (half_width is None):
        raise ValueError("gbp_sibson_pool: log_mean_prior and half_width come together")
    u = lmp = None
    if log_mean_prior is not None:
        lmp = np.array(host(log_mean_prior), dtype=np.float64)
        if lmp.shape != (N,) or not np.all(np.isfinite(lmp)):
            raise ValueError("gbp_sibson_pool: log_mean_prior must hold %d finite values" % N)
        if not (np.isfinite(float(half_width)) and float(half_width) > 0.0):
            raise ValueError("gbp_sibson_pool: half_width must be finite and positive")
        u = axis_offsets(lmp, half_width, nv)
    if max_total is not None and (int(max_total) != max_total or int(max_total) < 0):
        raise ValueError("gbp_sibson_pool: max_total is a count, got %r" % (max_total,))
    if out is not None:
        for k, shape, dt in (("pooled", (nv, nz), torch.int32), ("clipped", (nz,), torch.int64)):
            b = out[k]
            if b.dtype != dt or tuple(b.shape[1:]) != shape or b.shape[0] < pix.size or not b.is_contiguous() or b.device != maps.device:
                raise ValueError("gbp_sibson_pool: out[%r] must be a contiguous %s buffer [>= %d, %s] beside the maps" % (
                    k, dt, pix.size, ", ".join(str(s) for s in shape)))
    return pix, u, lmp


class SibsonPlan:
    """The geometry of one grid and one set of soundings: ``index`` (the nearest sounding of every pixel's node), ``distance`` (D) and
    ``count`` (n, the number of pixels covering a pixel), each an int32 ``[ny, nx]`` tensor on the device, and the cover lists the
    library keeps.  ``max_distance`` (metres; None / 0 / False: no mask) is the reference's ``mask``.  ``list_budget_bytes`` bounds the
    memory of the lists (default 4 GiB): beyond it the plan works in bands of destination rows, with the same results.

    ``x`` / ``y`` / edges: host arrays (or tensors, read on the host).  ``device``: default cuda:0."""

    def __init__(self, x, y, x_edges, y_edges, max_distance=None, device=None, list_budget_bytes=0):
        dev = torch.device(device) if device is not None else torch.device("cuda", 0)
        if dev.type != "cuda":
            raise _lib.NativeLibraryError("SibsonPlan runs on the device (gbp_sibson_plan_create); there is no host fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        px, py, dx, dy = pixel_coordinates(host(x), host(y), host(x_edges), host(y_edges))
        if not np.all(np.isfinite(px)) or not np.all(np.isfinite(py)):
            raise ValueError("the soundings' coordinates must be finite")
        md = float("inf") if not max_distance else float(max_distance)
        if not md > 0.0:
            raise ValueError("max_distance must be positive (None for no mask)")
        self.x_edges, self.y_edges = np.asarray(host(x_edges), dtype=np.float64), np.asarray(host(y_edges), dtype=np.float64)
        self.nx, self.ny, self.n_soundings = self.x_edges.size - 1, self.y_edges.size - 1, px.size
        self.max_distance_px2 = md / (dx * dy)
        self.device = dev
        self._handle = ctypes.c_void_p()
        lib = _lib.load()
        with torch.cuda.device(dev):
            tpx, tpy = torch.as_tensor(px).to(dev), torch.as_tensor(py).to(dev)
            _lib.check(lib.gbp_sibson_plan_create_ex(px.size, tpx.data_ptr(), tpy.data_ptr(), self.nx, self.ny, self.max_distance_px2,
                                                     int(list_budget_bytes), _lib.stream(dev), ctypes.byref(self._handle)))
        self.index = torch.empty((self.ny, self.nx), dtype=torch.int32, device=dev)
        self.distance = torch.empty_like(self.index)
        self.count = torch.empty_like(self.index)
        info = (ctypes.c_int64 * 4)()
        _lib.call("gbp_sibson_plan_query", dev, self._handle, self.index, self.distance, self.count, info)
        self.list_length, self.longest_list, self.n_bands, self.bytes_held = (int(v) for v in info)

    def apply(self, values):
        """``values`` [N] or [N, C] float64 on the plan's device -> [ny, nx] or [C, ny, nx]: per pixel the average of the values its
        covering pixels point at, summed in their row-major order; NaN where nothing covers the pixel or the mask applies; NaN values
        propagate."""
        if not torch.is_tensor(values) or values.device.type != "cuda":
            raise _lib.NativeLibraryError("SibsonPlan.apply runs on the device (gbp_sibson_apply); there is no host fallback")
        if values.device != self.device:
            raise ValueError("values are on %s, the plan on %s" % (values.device, self.device))
        if values.dtype != torch.float64 or values.dim() not in (1, 2) or values.shape[0] != self.n_soundings:
            raise ValueError("values must be float64 [N] or [N, C] with N = %d soundings, got %s %r" % (
                self.n_soundings, values.dtype, tuple(values.shape)))
        v = values.reshape(self.n_soundings, -1).contiguous()
        C = v.shape[1]
        if C < 1:
            raise ValueError("values hold no column")
        out = torch.empty((C, self.ny, self.nx), dtype=torch.float64, device=self.device)
        _lib.call("gbp_sibson_apply", self.device, self._handle, C, v, out)
        return out[0] if values.dim() == 1 else out

    def pool(self, maps, pixels=None, log_mean_prior=None, half_width=None, max_total=None, out=None):
        """Pixel posteriors (gbp_sibson_pool; DESIGN.md 3.19, the host statement of the rule is ``pixel_posteriors.pool_reference``):
        ``maps`` int32 [N, n_value, n_depth] on the plan's device -> dict(``pooled`` int32 [P, n_value, n_depth], the sum of the maps
        of each pixel's list; ``clipped`` int64 [P, n_depth], the counts that fell off the value axis; ``log_mean_prior`` [P], the
        pixel's axis = its nearest sounding's (None without one); ``count`` int32 [P], the entries pooled: the list's length, 0 under
        the mask).  ``pixels``: flat pixel numbers i * nx + j in any order, repeats allowed; None: every pixel in row-major order.
        ``log_mean_prior`` [N] (ln S/m, as ``hitmap.products`` takes it) and ``half_width`` come together: every sounding's value
        axis is centred on its own prior mean, and a neighbour's counts are moved by the nearest whole number of value cells onto the
        axis of the pixel's nearest sounding, whose own counts are never moved; without them nothing moves.  An entry adds its
        sounding's counts as they are: a sounding with more samples weighs more, one that never burned in (an empty map) weighs
        nothing.  ``max_total``: a bound of every column's total the caller knows (a chain's sample count), else found by one more
        read of the maps; a plan whose longest list times it could pass 2^31 - 1 in a pooled int32 cell is refused, and so is a
        banded plan.  ``out``: a dict(pooled, clipped) of buffers with room for P pixels to write into (views of them come back)."""
        pix, u, lmp = _pool_arguments(self, maps, pixels, log_mean_prior, half_width, max_total, out)
        if maps.device.type != "cuda":
            raise _lib.NativeLibraryError("SibsonPlan.pool runs on the device (gbp_sibson_pool); there is no host fallback")
        if maps.device != self.device:
            raise ValueError("gbp_sibson_pool: the maps are on %s, the plan on %s" % (maps.device, self.device))
        dev = self.device
        _, nv, nz = maps.shape
        P = pix.size
        if max_total is None:
            max_total = int(maps.sum(dim=1, dtype=torch.int64).max()) if maps.numel() else 0
        with torch.cuda.device(dev):
            pix_d = torch.as_tensor(pix.astype(np.int32)).to(dev)
            u_d = None if u is None else torch.as_tensor(u).to(dev)
            if out is None:
                pooled = torch.empty((P, nv, nz), dtype=torch.int32, device=dev)
                clipped = torch.empty((P, nz), dtype=torch.int64, device=dev)
            else:
                pooled, clipped = out["pooled"][:P], out["clipped"][:P]
            _lib.call("gbp_sibson_pool", dev, self._handle, P, pix_d, nv, nz, maps, u_d, int(max_total), pooled, clipped)
            where = pix_d.long()
            near = self.index.reshape(-1)[where].long()
            d = self.distance.reshape(-1)[where].to(torch.float64)
            count = torch.where(d * d + 0.25 > self.max_distance_px2, torch.zeros_like(where, dtype=torch.int32), self.count.reshape(-1)[where])
            lmp_p = None if lmp is None else torch.as_tensor(lmp).to(dev)[near]
        return dict(pooled=pooled, clipped=clipped, log_mean_prior=lmp_p, count=count)

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().gbp_sibson_plan_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sibson(x, y, values, x_edges, y_edges, max_distance=None):
    """The reference's ``sibson(x, y, values, grid_x, grid_y, max_distance=...)`` for ``values`` [N] or [N, C] on the device: one plan,
    one apply."""
    if not torch.is_tensor(values) or values.device.type != "cuda":
        raise _lib.NativeLibraryError("gridding.sibson runs on the device (gbp_sibson_apply); there is no host fallback")
    plan = SibsonPlan(x, y, x_edges, y_edges, max_distance=max_distance, device=values.device)
    try:
        return plan.apply(values)
    finally:
        torch.cuda.synchronize(values.device)
        plan.close()
