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


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


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
        px, py, dx, dy = pixel_coordinates(_host(x), _host(y), _host(x_edges), _host(y_edges))
        if not np.all(np.isfinite(px)) or not np.all(np.isfinite(py)):
            raise ValueError("the soundings' coordinates must be finite")
        md = float("inf") if not max_distance else float(max_distance)
        if not md > 0.0:
            raise ValueError("max_distance must be positive (None for no mask)")
        self.x_edges, self.y_edges = np.asarray(_host(x_edges), dtype=np.float64), np.asarray(_host(y_edges), dtype=np.float64)
        self.nx, self.ny, self.n_soundings = self.x_edges.size - 1, self.y_edges.size - 1, px.size
        self.max_distance_px2 = md / (dx * dy)
        self.device = dev
        self._handle = ctypes.c_void_p()
        lib = _lib.load()
        with torch.cuda.device(dev):
            tpx, tpy = torch.as_tensor(px).to(dev), torch.as_tensor(py).to(dev)
            _lib.check(lib.gbp_sibson_plan_create_ex(px.size, tpx.data_ptr(), tpy.data_ptr(), self.nx, self.ny, self.max_distance_px2,
                                                     int(list_budget_bytes), torch.cuda.current_stream(dev).cuda_stream,
                                                     ctypes.byref(self._handle)))
            self.index = torch.empty((self.ny, self.nx), dtype=torch.int32, device=dev)
            self.distance = torch.empty_like(self.index)
            self.count = torch.empty_like(self.index)
            info = (ctypes.c_int64 * 4)()
            _lib.check(lib.gbp_sibson_plan_query(self._handle, self.index.data_ptr(), self.distance.data_ptr(), self.count.data_ptr(), info,
                                                 torch.cuda.current_stream(dev).cuda_stream))
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
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gbp_sibson_apply(self._handle, C, v.data_ptr(), out.data_ptr(),
                                                    torch.cuda.current_stream(self.device).cuda_stream))
        return out[0] if values.dim() == 1 else out

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
