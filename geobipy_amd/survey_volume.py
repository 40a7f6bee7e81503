"""Survey volumes: the line products of ALL flight lines of a survey on one regular x-y grid, depth cell by depth cell -- depth-slice
maps and 3-D volumes, what the reference's ``Inference3D.interpolate_3d`` / ``map_depth_slice`` / ``interpolate_marginal_3d`` build
through ``Point.interpolate(method='sibson')`` (inversion/Inference3D.py -> pointcloud/Point.py -> base/interpolation.py).

The reference grids one depth cell of one variable at a time, each a full sweep of the raster.  Here the soundings of every line are
concatenated in line order, ONE ``gridding.SibsonPlan`` holds the geometry of the grid, and the plan is applied to ``[N, columns]`` blocks
of each variable (columns = depth cells; ``class_probability`` [N, K, n_depth] goes through as K n_depth columns).  The grid is the
reference's centred mesh over the soundings' bounding box (``gridding.centred_mesh``); the depth axis is the first line's, and every
other line must share it (the reference takes ``lines[0].mesh.y`` for all, ``Inference3D.zGrid``).  ``elevation`` [ny, nx] is the
soundings' elevation through the same plan -- the reference's ``mesh3d`` drapes its surface with ``Point.interpolate``'s default
method (minimum curvature); this one is the Sibson surface.

    python -m geobipy_amd.survey_volume <directory> --dx DX --dy DY [--variables mean percentile_5 ...] [--mask MAX_DISTANCE]
                                        [--depth D | --depth-cells I0 I1 | --elevation-axis DZ [TOP BOTTOM] | --elevation E
                                         | --depth-intervals E0 E1 ... | --elevation-intervals E0 E1 ...]
                                        [--pooled] [--block COLUMNS] [--device cuda:0] [--out DIRECTORY]

reads the directory's line containers and their ``<line>.products.npz`` (computed where absent: ``line_products.from_results``) and writes
``survey_volume.npz`` (x_edges, y_edges, depth_edges, elevation, count, nearest_distance, the variables' names) and one
``survey_volume.<variable>.npy`` [n_depth, ny, nx] per variable, filled column block by column block through a memory map: a volume is
n_depth ny nx 8 bytes (440 x 1 000 x 1 000: 3.5 GB) and is never held in memory whole.

Those volumes hang under the terrain: index 0 is the first depth cell below ``elevation`` [ny, nx], another horizon at every pixel.  With
``--elevation-axis`` (``from_lines(elevation_edges=...)``) every sounding's column is first resampled from its depth cells onto ONE
elevation axis (``elevation.resample``, csrc/gbp_elev.h: the reference's ``Inference2D.elevationSlice``), block of elevation cells by
block on the device, and then gridded by the same plan: ``survey_volume.<variable>.npy`` is [n_elev, ny, nx] with index 0 the LOWEST
cell and a regular z axis (``elevation_edges`` in ``survey_volume.npz``), a voxel model as it stands.  ``--elevation E`` is one
horizontal slice [ny, nx] at that elevation.  The reference slices first and grids afterwards, and so does this: a sounding that is
outside its own mesh at a level (above its surface, below its last depth edge) is NaN there, NaN propagates through the Sibson sum, and
so a pixel is NaN at a level wherever ANY sounding that contributes to it is outside its mesh -- the volume's top follows the terrain
from below and its bottom the deepest common reach.

With ``--depth-intervals`` / ``--elevation-intervals`` (``from_lines(intervals=...)``) the maps are of UNITS: per variable [M, ny, nx],
map m the statistic of the marginal posterior of the unit between edges m and m + 1 (the lines' ``interval_*`` products,
geobipy_amd/intervals.py), in ``survey_volume.intervals.<variable>.npy`` beside ``survey_volume.intervals.npz``.

With ``--pooled`` (``from_lines(pooled=True)``) nothing is gridded: every pixel gets a posterior of its own, the pool of its natural
neighbours' hit maps through the same plan (geobipy_amd/pixel_posteriors.py), and the variables are the products of that posterior, in
``survey_volume.pooled.<variable>.npy`` [n_depth, ny, nx].
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch

from . import elevation as elevation_axis
from . import gridding, line_products

AXES_FILE = "survey_volume.npz"
INTERVALS_AXES_FILE = "survey_volume.intervals.npz"


def volume_path(directory, variable):
    return os.path.join(str(directory), "survey_volume.%s.npy" % variable)


def pooled_volume_path(directory, variable):
    """The file of a variable taken from the pixel posteriors (``from_lines(pooled=True)``): it carries ``pooled``."""
    return os.path.join(str(directory), "survey_volume.pooled.%s.npy" % variable)


def intervals_volume_path(directory, variable):
    """The file of a variable's interval maps [M, ny, nx]: it carries ``intervals``, these maps have no depth axis."""
    return os.path.join(str(directory), "survey_volume.intervals.%s.npy" % variable)


def depth_cells(depth, depth_edges):
    """The depth cells ``depth`` selects, as a slice (``Inference2D._z_slice``): None -> all; an int -> that cell; a float -> the cell
    holding that depth (m); a slice -> itself; a pair of ints -> cells i0 .. i1 inclusive; a pair of floats -> the cells holding both
    depths and those between."""
    e = np.asarray(depth_edges, dtype=np.float64)
    nz = e.size - 1

    def cell(d):
        if not e[0] <= float(d) < e[-1]:
            raise ValueError("depth %g is outside the depth axis [%g, %g)" % (d, e[0], e[-1]))
        return int(np.searchsorted(e, float(d), side="right")) - 1

    def index(i):
        if not -nz <= int(i) < nz:
            raise ValueError("depth cell %d is outside 0 .. %d" % (i, nz - 1))
        return int(i) % nz

    if depth is None:
        return slice(0, nz)
    if isinstance(depth, slice):
        return slice(*depth.indices(nz))
    if isinstance(depth, (int, np.integer)):
        return slice(index(depth), index(depth) + 1)
    if np.size(depth) == 1:
        c = cell(np.asarray(depth).reshape(-1)[0])
        return slice(c, c + 1)
    if np.size(depth) != 2:
        raise ValueError("depth must be a cell, a depth, a slice or a pair")
    a, b = depth
    ints = all(isinstance(v, (int, np.integer)) for v in (a, b))
    lo, hi = sorted((index(a), index(b)) if ints else (cell(a), cell(b)))
    return slice(lo, hi + 1)


def load_line(path, device=None, block=4096, intervals=None, classes=None, variables=()):
    """(x, y, elevation, products) of one line container: the soundings' coordinates from /data/x, /data/y, /data/elevation and the line
    products from ``<line>.products.npz`` where present, else computed (``line_products.from_results``).  With ``intervals`` (a checked
    spec, ``intervals.check_spec``) the saved file is used only if it holds interval entries for the identical spec; otherwise the line
    and every one of ``variables`` as ``interval_<variable>``; otherwise the line is computed from its container, with ``classes``
    where given."""
    from . import hdf
    from . import intervals as iv
    arrays, _ = hdf.load_results(path)
    x = line_products._key(arrays, "/data/x/data", "/data/x")
    y = line_products._key(arrays, "/data/y/data", "/data/y")
    if x is None or y is None:
        raise ValueError("%s holds no /data/x and /data/y" % path)
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    elev = line_products._key(arrays, "/data/elevation/data", "/data/elevation")
    elev = np.zeros_like(x) if elev is None else np.asarray(elev, dtype=np.float64).reshape(-1)
    saved = line_products.output_path(path)
    prod = None
    if os.path.exists(saved):
        with np.load(saved) as z:
            prod = {k: z[k] for k in z.files}
        if intervals is not None and not (iv.same_spec(prod, intervals) and all("interval_" + v in prod for v in variables)):
            prod = None
    if prod is None:
        prod = line_products.from_results(path, device=device, block=block, intervals=intervals, classes=classes)
    if prod["mean"].shape[0] != x.size or elev.size != x.size:
        raise ValueError("%s: %d soundings but products for %d" % (path, x.size, prod["mean"].shape[0]))
    return x, y, elev, prod


def _columns(prod_per_line, name, n_depth):
    """([N, K, n_depth], whether the variable has a class axis) of variable ``name`` over all lines, line after line (K = 1 for the
    [N, n_depth] variables)."""
    if name.startswith("interval_"):
        raise ValueError("%r is a variable of units, not of depth cells: grid it with intervals=..." % name)
    parts, ndim = [], set()
    for path, prod in prod_per_line:
        if name not in prod:
            raise ValueError("%s: the line products hold no %r (present: %s)" % (path, name, ", ".join(sorted(prod))))
        a = np.asarray(prod[name], dtype=np.float64)
        if a.ndim not in (2, 3) or a.shape[-1] != n_depth:
            raise ValueError("%s: %r is not a per-depth-cell variable (shape %r)" % (path, name, a.shape))
        parts.append(a.reshape(a.shape[0], -1, n_depth))
        ndim.add(a.ndim)
    if len({p.shape[1] for p in parts}) != 1 or len(ndim) != 1:
        raise ValueError("%r has a different number of classes from line to line" % name)
    return np.concatenate(parts), ndim == {3}


def _on_elevation(plan, lines, name, surface, d_edges, mode, axis, block, out):
    """The volume of variable ``name`` on the elevation axis (``mode``, ``axis``: ``elevation.check_axis``): [n_elev, ny, nx] for
    cells, [ny, nx] for the one level, a leading class axis where the variable has one; a memory map under ``out``."""
    if mode == elevation_axis.INTERVALS:
        for ln in lines:
            if name in ln[4] and np.asarray(ln[4][name]).dtype.kind in "iub":
                raise ValueError("%s: %r holds integers (class indices), and their mean over elevation cells means nothing: take one "
                                 "level (elevation=...) or grid class_probability" % (ln[0], name))
    cols, with_classes = _columns([(ln[0], ln[4]) for ln in lines], name, d_edges.size - 1)     # [N, K, n_depth]
    K, n_elev, ny, nx = cols.shape[1], axis.size - (mode == elevation_axis.INTERVALS), plan.ny, plan.nx
    shape = ((K,) if with_classes else ()) + ((n_elev,) if mode == elevation_axis.INTERVALS else ()) + (ny, nx)
    if out is not None:
        vol = np.lib.format.open_memmap(volume_path(out, name), mode="w+", dtype=np.float64, shape=shape)
    else:
        vol = np.empty(shape, dtype=np.float64)
    cube = vol.reshape(K, n_elev, ny, nx)
    v = torch.as_tensor(cols).to(plan.device)                                                    # once per variable
    key = "edges" if mode == elevation_axis.INTERVALS else "levels"
    for c0 in range(0, n_elev, block):
        c1 = min(n_elev, c0 + block)
        r = elevation_axis.resample(v, surface, d_edges, columns=(c0, c1), **{key: axis})       # [N, K, c1 - c0]
        cube[:, c0:c1] = plan.apply(r.reshape(r.shape[0], K * (c1 - c0))).reshape(K, c1 - c0, ny, nx).cpu().numpy()
    if out is not None:
        vol.flush()
    return vol


def _interval_columns(prod_per_line, name, M):
    """([N, K, M], whether the variable has a class axis) of the unit variable ``interval_<name>`` over all lines."""
    key = "interval_" + name
    parts, ndim = [], set()
    for path, prod in prod_per_line:
        if key not in prod:
            raise ValueError("%s: the line products hold no %r (present: %s)" % (path, key, ", ".join(sorted(k for k in prod if k.startswith("interval_")))))
        a = np.asarray(prod[key], dtype=np.float64)
        if a.ndim not in (2, 3) or a.shape[-1] != M:
            raise ValueError("%s: %r is not a per-unit variable (shape %r)" % (path, key, a.shape))
        parts.append(a.reshape(a.shape[0], -1, M))
        ndim.add(a.ndim)
    if len({p.shape[1] for p in parts}) != 1 or len(ndim) != 1:
        raise ValueError("%r has a different number of classes from line to line" % key)
    return np.concatenate(parts), ndim == {3}


def load_maps(path):
    """(x, y, elevation, hit maps int32 [N, n_value, n_depth], log_mean_prior [N] (ln S/m), half_width, depth_edges) of one line
    container, on the host: what ``line_products.from_results`` uploads block by block."""
    from . import hdf
    arrays, _ = hdf.load_results(path)
    x = line_products._key(arrays, "/data/x/data", "/data/x")
    y = line_products._key(arrays, "/data/y/data", "/data/y")
    if x is None or y is None:
        raise ValueError("%s holds no /data/x and /data/y" % path)
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    elev = line_products._key(arrays, "/data/elevation/data", "/data/elevation")
    elev = np.zeros_like(x) if elev is None else np.asarray(elev, dtype=np.float64).reshape(-1)
    V = line_products.VALUES
    hm = line_products._key(arrays, V + "/values/data", V + "/values")
    if hm is None or hm.ndim != 3:
        raise ValueError("%s holds no conductivity-depth hit maps [N, n_value, n_depth] at %s" % (path, V))
    v_edges = line_products._key(arrays, V + "/mesh/y/edges/data")
    d_edges = line_products._key(arrays, V + "/mesh/z/edges/data")
    rel = line_products._key(arrays, V + "/mesh/y/relative_to/data")
    N, nv, nz = hm.shape
    if v_edges is None or d_edges is None or v_edges.size != nv + 1 or d_edges.size != nz + 1:
        raise ValueError("%s: the hit maps' mesh (%s/mesh/y and /z edges) does not match their shape %r" % (path, V, hm.shape))
    if x.size != N or elev.size != N:
        raise ValueError("%s: %d soundings but hit maps for %d" % (path, x.size, N))
    hw = line_products._uniform_half_width(v_edges)
    rel = np.zeros(N) if rel is None else np.broadcast_to(np.asarray(rel, dtype=np.float64).reshape(-1), (N,))
    return x, y, elev, hm, rel * line_products.LN10, hw, np.asarray(d_edges, dtype=np.float64)


def pooled_variables(variables, classes=None):
    """(names, percentiles) of the ``variables`` a pooled volume may hold, checked by name: ``pixel_posteriors.VARIABLES`` and
    percentile_<p>; the percentiles to ask ``pixel_posteriors.products`` for."""
    from . import pixel_posteriors as pp
    pct = []
    for name in variables:
        if name.startswith("percentile_"):
            try:
                p = float(name[len("percentile_"):])
            except ValueError:
                p = float("nan")
            if not 0.0 < p < 100.0 or pp.percentile_name(p) != name:
                raise ValueError("%r is not percentile_<p> with p in (0, 100), written as %%g writes it" % name)
            pct.append(p)
        elif name not in pp.VARIABLES:
            raise ValueError("%r cannot be taken from the pixel posteriors (pooled): %s or percentile_<p>" % (name, ", ".join(pp.VARIABLES)))
        elif name in ("class_probability", "highest_marginal") and classes is None:
            raise ValueError("%r needs classes=(means, scales)" % name)
    return list(variables), tuple(pct) if pct else (50.0,)


def _pooled_from_lines(paths, dx, dy, variables, max_distance, depth, block, device, out, list_budget_bytes, classes):
    """``from_lines(pooled=True)``: the variables from the pixel posteriors (geobipy_amd/pixel_posteriors.py), block of pixels by block."""
    from . import pixel_posteriors as pp
    names, pct = pooled_variables(variables, classes)
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = [f for p in paths for f in line_products.containers(str(p))]
    if not files:
        raise ValueError("no results containers under %s" % " ".join(str(p) for p in paths))
    if int(block) < 1:
        raise ValueError("block must be positive")
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    lines = [(f,) + load_maps(f) for f in files]
    d_edges, hw, shape = lines[0][7], lines[0][6], lines[0][4].shape[1:]
    for ln in lines[1:]:
        if not np.array_equal(ln[7], d_edges):
            raise ValueError("%s does not share the depth mesh of %s" % (ln[0], lines[0][0]))
        if ln[4].shape[1:] != shape or ln[6] != hw:
            raise ValueError("%s does not share the value axis of %s (%r cells of half width %g)" % (ln[0], lines[0][0], shape[0], hw))
    nv, nz = shape
    cells = depth_cells(depth, d_edges)
    single = depth is not None and not isinstance(depth, slice) and np.size(depth) == 1
    x, y, elev = (np.concatenate([ln[k] for ln in lines]) for k in (1, 2, 3))
    lmp = np.concatenate([ln[5] for ln in lines])
    need = x.size * nv * nz * 4
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise ValueError("pooled: the hit maps of all lines must be resident at once, %d soundings x %d x %d cells x 4 bytes = %d bytes, "
                         "and the device has %d bytes free" % (x.size, nv, nz, need, free))
    x_edges, y_edges = gridding.centred_mesh(x, y, dx, dy)
    plan = gridding.SibsonPlan(x, y, x_edges, y_edges, max_distance=max_distance, device=dev, list_budget_bytes=list_budget_bytes)
    try:
        if plan.n_bands > 1:
            raise ValueError("pooled: the plan is banded (%d bands under list_budget_bytes), and pooling needs every list resident" % plan.n_bands)
        ny, nx = plan.ny, plan.nx
        res = dict(x_edges=x_edges, y_edges=y_edges, depth_edges=d_edges[cells.start:cells.stop + 1], x=x, y=y,
                   elevation=plan.apply(torch.as_tensor(elev).to(plan.device)).cpu().numpy(), count=plan.count.cpu().numpy(),
                   nearest_distance=plan.distance.cpu().numpy(), variables=np.array(names), pooled=np.bool_(True))
        if out is not None:
            os.makedirs(str(out), exist_ok=True)
            np.savez(os.path.join(str(out), AXES_FILE), **res)
        maps = torch.cat([torch.as_tensor(np.ascontiguousarray(ln[4], dtype=np.int32)).to(dev) for ln in lines])
        ncell, P = cells.stop - cells.start, nx * ny
        flats = {}
        for name in names:
            K = () if name != "class_probability" else (len(classes[0]),)
            shape = K + (() if single else (ncell,)) + (ny, nx)
            dtype = np.int32 if name == "highest_marginal" else np.float64
            if out is not None:
                res[name] = np.lib.format.open_memmap(pooled_volume_path(out, name), mode="w+", dtype=dtype, shape=shape)
            else:
                res[name] = np.empty(shape, dtype=dtype)
            flats[name] = res[name].reshape(K + (ncell, P))
        moments = None                                                                       # total, s1 of every pixel: the entropy's
        if "entropy" in names:
            moments = (torch.empty((P, nz), dtype=torch.int64, device=dev), torch.empty((P, nz), dtype=torch.float64, device=dev))
        for p0, _, r in pp.blocks(plan, maps, lmp, hw, block=int(block), percentiles=pct, credible=90.0, classes=classes, depth_edges=d_edges):
            b = r["total"].shape[0]
            if moments is not None:
                moments[0][p0:p0 + b], moments[1][p0:p0 + b] = r["total"], r["s1"]
            for name in names:
                if name != "entropy":
                    v = r[name][..., cells].cpu().numpy()                                    # [b, cells] or [b, K, cells]
                    flats[name][..., p0:p0 + b] = np.moveaxis(v, 0, -1)
        if moments is not None:
            flats["entropy"][:] = pp.entropy(moments[0], moments[1], nv, hw, d_edges)[:, cells].cpu().numpy().T
        if out is not None:
            for name in names:
                res[name].flush()
    finally:
        torch.cuda.synchronize(plan.device)
        plan.close()
    return res


def from_lines(paths, dx, dy, variables=("mean",), max_distance=None, depth=None, block=256, device=None, out=None,
               list_budget_bytes=0, elevation_edges=None, elevation=None, intervals=None, classes=None, pooled=False):
    """Grid the line products of the containers ``paths`` (a directory, a container or a list of them; the lines in sorted order).

    Returns a dict: ``x_edges``, ``y_edges`` (``gridding.centred_mesh`` of all soundings at spacing ``dx``, ``dy``), ``depth_edges``
    (of the selected cells), ``elevation`` [ny, nx], ``count`` (n, the number of pixels covering a pixel) and ``nearest_distance`` (D,
    pixels) [ny, nx], ``x``, ``y`` (the soundings), and per variable an array [n_depth, ny, nx] ([K, n_depth, ny, nx] for
    ``class_probability``; [ny, nx] / [K, ny, nx] when ``depth`` selects one cell).  ``depth``: see ``depth_cells``.
    ``max_distance`` (m) masks the pixels far from any sounding (``gridding``).  ``block`` columns go through the device at a time.
    With ``out`` (a directory) the axes go to ``survey_volume.npz`` and each variable to ``survey_volume.<variable>.npy`` through a
    memory map, and the returned arrays of the variables are those maps.

    ``elevation_edges`` (ascending edges [n_elev + 1] in m, or a function (surface elevations [N], depth_edges) -> such edges, e.g.
    ``functools.partial(elevation.regular_axis, dz=2.0)``) puts the volumes on that elevation axis instead of the depth axis: every
    variable goes to the device once as [N, K, n_depth], ``block`` elevation cells at a time are resampled there
    (``elevation.resample``: the mean of the depth cells each elevation cell overlaps, per sounding under its own surface elevation) and
    put through the plan.  The variables come back as [n_elev, ny, nx] ([K, n_elev, ny, nx] with classes), index 0 the lowest cell, and
    the result gains ``elevation_edges``.  ``elevation`` (a number, m) is one horizontal slice, the value of the depth cell holding that
    level under each sounding: [ny, nx] ([K, ny, nx]), and the result gains ``elevation_level``.  Both exclude ``depth`` and each
    other; ``depth_edges`` (whole) and the draped ``elevation`` surface stay in the result.  The reference slices, then grids
    (``Inference2D.elevationSlice``, then ``Point.interpolate``), so a pixel is NaN at a level wherever any sounding contributing to it
    is outside its own mesh there: NaN propagates through the Sibson sum.  Integer line products (class indices) are refused on an
    elevation axis -- their mean means nothing; a single ``elevation`` level takes them.

    ``intervals`` (a spec of kind depth, pairs or elevation: ``line_products.from_results``, geobipy_amd/intervals.py) grids the
    products of M UNITS instead of depth cells: variable ``mean`` is the lines' ``interval_mean`` [N, M] (the statistic of each unit's
    marginal posterior), and comes back as [M, ny, nx] ([K, M, ny, nx] for ``class_probability``) through the same plan, with the
    spec (``interval_kind``, ``interval_edges`` / ``interval_pairs``) in the result; the files are ``survey_volume.intervals.npz`` and
    ``survey_volume.intervals.<variable>.npy``.  It excludes ``depth``, ``elevation_edges`` and ``elevation``.  A line's saved products
    are used only if they hold interval entries for the identical spec; otherwise the line is computed from its container (``classes``
    = (means, scales) where ``class_probability`` is asked for).  A pixel is NaN for a unit wherever any contributing sounding has no
    cell of the unit.  Horizons differ from line to line: compute them per line (``from_results``).

    ``pooled=True`` takes the variables from the PIXEL POSTERIORS instead of gridding them (geobipy_amd/pixel_posteriors.py, DESIGN.md
    3.19): every pixel's posterior is the pool of its natural neighbours' hit maps through the same plan, and ``mean``, ``median``,
    ``mode``, ``percentile_<p>``, ``credible_low`` / ``_high`` / ``_range`` (90 %), ``entropy``, ``class_probability`` and
    ``highest_marginal`` (with ``classes``) and ``clipped_share`` are the products of that posterior; any other name is refused.  The
    hit maps of all lines are read from the containers and must be resident on the device at once (refused with the figure
    otherwise); ``block`` PIXELS go through at a time; the files are ``survey_volume.pooled.<variable>.npy`` [n_depth, ny, nx] and
    ``survey_volume.npz`` holds ``pooled`` = True.  ``depth`` selects cells as above (the entropy stays that of the whole column, and
    asking for it keeps two more [pixels, n_depth] arrays on the device).  A
    masked pixel holds what an empty column gives, not NaN.  ``elevation_edges``, ``elevation``, ``intervals`` and a banded plan are
    refused together with it."""
    if pooled:
        if elevation_edges is not None or elevation is not None or intervals is not None:
            raise ValueError("pooled excludes elevation_edges, elevation and intervals")
        return _pooled_from_lines(paths, dx, dy, variables, max_distance, depth, block, device, out, list_budget_bytes,
                                  None if classes is None else line_products.check_classes(*classes))
    on_axis, on_level = elevation_edges is not None, elevation is not None
    if intervals is not None:
        from . import intervals as iv
        if on_axis or on_level or depth is not None:
            raise ValueError("intervals excludes depth, elevation_edges and elevation")
        intervals = iv.check_spec(intervals)
        if intervals["kind"] == "horizons" or "surface" in intervals:
            raise ValueError("intervals over several lines: kind depth, pairs or elevation, the surface from each line's container")
    if on_axis and on_level:
        raise ValueError("elevation_edges and elevation exclude each other")
    if (on_axis or on_level) and depth is not None:
        raise ValueError("elevation_edges / elevation and depth exclude each other")
    if on_level and not (np.size(elevation) == 1 and np.isfinite(float(np.asarray(elevation).reshape(-1)[0]))):
        raise ValueError("elevation must be one finite level (m)")
    if on_axis and not callable(elevation_edges):
        elevation_axis.check_axis(edges=elevation_edges)
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = [f for p in paths for f in line_products.containers(str(p))]
    if not files:
        raise ValueError("no results containers under %s" % " ".join(str(p) for p in paths))
    if int(block) < 1:
        raise ValueError("block must be positive")
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    lines = [(f,) + load_line(f, device=dev, intervals=intervals, classes=classes, variables=tuple(variables)) for f in files]
    d_edges = np.asarray(lines[0][4]["depth_edges"], dtype=np.float64)
    for f, _, _, _, prod in lines[1:]:
        if not np.array_equal(np.asarray(prod["depth_edges"], dtype=np.float64), d_edges):
            raise ValueError("%s does not share the depth mesh of %s" % (f, lines[0][0]))
    nz = d_edges.size - 1
    cells = depth_cells(depth, d_edges)
    single = depth is not None and not isinstance(depth, slice) and np.size(depth) == 1
    x = np.concatenate([ln[1] for ln in lines])
    y = np.concatenate([ln[2] for ln in lines])
    elev = np.concatenate([ln[3] for ln in lines])
    x_edges, y_edges = gridding.centred_mesh(x, y, dx, dy)
    plan = gridding.SibsonPlan(x, y, x_edges, y_edges, max_distance=max_distance, device=dev, list_budget_bytes=list_budget_bytes)
    try:
        ny, nx = plan.ny, plan.nx
        res = dict(x_edges=x_edges, y_edges=y_edges, depth_edges=d_edges[cells.start:cells.stop + 1], x=x, y=y,
                   elevation=plan.apply(torch.as_tensor(elev).to(plan.device)).cpu().numpy(), count=plan.count.cpu().numpy(),
                   nearest_distance=plan.distance.cpu().numpy(), variables=np.array(list(variables)))
        if on_axis:
            mode, axis, _ = elevation_axis.check_axis(edges=elevation_edges(elev, d_edges) if callable(elevation_edges) else elevation_edges)
            res["elevation_edges"] = axis
        elif on_level:
            mode, axis, _ = elevation_axis.check_axis(levels=[float(np.asarray(elevation).reshape(-1)[0])])
            res["elevation_level"] = np.float64(axis[0])
        if intervals is not None:
            res.update(iv.describe(intervals))
        if out is not None:
            os.makedirs(str(out), exist_ok=True)
            np.savez(os.path.join(str(out), AXES_FILE if intervals is None else INTERVALS_AXES_FILE), **res)
        ncell = cells.stop - cells.start if intervals is None else iv.n_intervals(intervals)
        surface = torch.as_tensor(elev).to(plan.device) if (on_axis or on_level) else None
        for name in variables:
            if surface is not None:
                res[name] = _on_elevation(plan, lines, name, surface, d_edges, mode, axis, int(block), out)
                continue
            if intervals is not None:
                cols, with_classes = _interval_columns([(ln[0], ln[4]) for ln in lines], name, ncell)   # [N, K, M]
            else:
                cols, with_classes = _columns([(ln[0], ln[4]) for ln in lines], name, nz)
                cols = cols[:, :, cells]                                                         # [N, K, cells]
            K = cols.shape[1]
            shape = ((K,) if with_classes else ()) + (() if single else (ncell,)) + (ny, nx)
            if out is not None:
                vol = np.lib.format.open_memmap((volume_path if intervals is None else intervals_volume_path)(out, name), mode="w+",
                                                dtype=np.float64, shape=shape)
            else:
                vol = np.empty(shape, dtype=np.float64)
            flat = vol.reshape(K * ncell, ny, nx)
            flat_cols = cols.reshape(cols.shape[0], K * ncell)
            for c0 in range(0, K * ncell, int(block)):
                c1 = min(K * ncell, c0 + int(block))
                v = torch.as_tensor(np.ascontiguousarray(flat_cols[:, c0:c1])).to(plan.device)
                flat[c0:c1] = plan.apply(v).cpu().numpy()
            if out is not None:
                vol.flush()
            res[name] = vol
    finally:
        torch.cuda.synchronize(plan.device)
        plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(prog="python -m geobipy_amd.survey_volume",
                                 description="Grid the line products of a directory of GeoBIPy results containers onto a regular x-y "
                                             "raster by discrete Sibson interpolation, depth cell by depth cell: survey_volume.npz (axes, "
                                             "elevation, count, nearest_distance) and survey_volume.<variable>.npy per variable.")
    ap.add_argument("paths", nargs="+", help="directories holding <line>.h5 / <line>.results.npz, or such containers")
    ap.add_argument("--dx", type=float, required=True, help="grid spacing in x (m)")
    ap.add_argument("--dy", type=float, required=True, help="grid spacing in y (m)")
    ap.add_argument("--variables", nargs="+", default=["mean"], metavar="NAME",
                    help="line products to grid (default mean): mean median mode percentile_<p> credible_range entropy opacity "
                         "interface_probability class_probability ...")
    ap.add_argument("--mask", type=float, default=None, metavar="MAX_DISTANCE", help="mask pixels farther than this from any sounding (m)")
    ap.add_argument("--depth", type=float, default=None, metavar="D", help="one map: the depth cell holding depth D (m)")
    ap.add_argument("--depth-cells", type=int, nargs=2, default=None, metavar=("I0", "I1"), help="the depth cells I0 .. I1 (inclusive) only")
    ap.add_argument("--elevation-axis", type=float, nargs="+", default=None, metavar="DZ [TOP BOTTOM]",
                    help="volumes on a regular elevation axis of DZ m instead of the depth axis, from BOTTOM to TOP (default: everything "
                         "the soundings reach), snapped outward to multiples of DZ; index 0 is the lowest cell")
    ap.add_argument("--elevation", type=float, default=None, metavar="E", help="one map: the horizontal slice at elevation E (m)")
    line_products.add_interval_arguments(ap)
    ap.add_argument("--pooled", action="store_true",
                    help="take the variables from the pixel posteriors (every pixel's pool of its natural neighbours' hit maps) instead of "
                         "gridding them: survey_volume.pooled.<variable>.npy; mean median mode percentile_<p> credible_low credible_high "
                         "credible_range entropy clipped_share; --block is then in pixels")
    ap.add_argument("--block", type=int, default=256, help="columns per pass through the device (default 256)")
    ap.add_argument("--device", default=None, help="torch device of the kernels (default cuda:0)")
    ap.add_argument("--out", default=None, help="directory of the outputs (default: the first path's directory)")
    return ap


def parse_args(argv=None):
    """The command line's arguments, checked: positive spacings, mask and block, at most one of --depth, --depth-cells, --elevation-axis
    and --elevation, 0 <= I0 <= I1, DZ > 0 and BOTTOM < TOP."""
    ap = parser()
    a = ap.parse_args(argv)
    for name, v in (("--dx", a.dx), ("--dy", a.dy)):
        if not (v > 0.0 and np.isfinite(v)):
            ap.error("%s must be positive and finite, got %g" % (name, v))
    if a.mask is not None and not (a.mask > 0.0 and np.isfinite(a.mask)):
        ap.error("--mask must be positive and finite")
    if a.depth is not None and a.depth_cells is not None:
        ap.error("--depth and --depth-cells exclude each other")
    if sum(v is not None for v in (a.depth, a.depth_cells, a.elevation_axis, a.elevation)) > 1:
        ap.error("--depth, --depth-cells, --elevation-axis and --elevation exclude one another")
    if a.elevation is not None and not np.isfinite(a.elevation):
        ap.error("--elevation must be finite")
    if a.elevation_axis is not None:
        try:
            line_products.elevation_axis_arguments(a.elevation_axis)
        except ValueError as e:
            ap.error("--elevation-axis: " + str(e))
    if a.depth is not None and not np.isfinite(a.depth):
        ap.error("--depth must be finite")
    if a.depth_cells is not None and not 0 <= a.depth_cells[0] <= a.depth_cells[1]:
        ap.error("--depth-cells needs 0 <= I0 <= I1")
    if a.block < 1:
        ap.error("--block must be positive")
    if len(set(a.variables)) != len(a.variables):
        ap.error("--variables holds a name twice")
    a.intervals = line_products.interval_arguments(ap, a, ("--depth", "--depth-cells", "--elevation-axis", "--elevation"))
    if a.pooled:
        for name, v in (("--elevation-axis", a.elevation_axis), ("--elevation", a.elevation), ("--depth-intervals", a.depth_intervals),
                        ("--elevation-intervals", a.elevation_intervals)):
            if v is not None:
                ap.error("--pooled and %s exclude each other" % name)
        try:
            pooled_variables(a.variables, classes=None)
        except ValueError as e:
            ap.error("--pooled: " + str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    depth = a.depth if a.depth is not None else (None if a.depth_cells is None else slice(a.depth_cells[0], a.depth_cells[1] + 1))
    out = a.out if a.out is not None else (a.paths[0] if os.path.isdir(a.paths[0]) else os.path.dirname(os.path.abspath(a.paths[0])))
    edges = None
    if a.elevation_axis is not None:
        dz, top, bottom = line_products.elevation_axis_arguments(a.elevation_axis)
        edges = functools.partial(elevation_axis.regular_axis, dz=dz, top=top, bottom=bottom)
    try:
        r = from_lines(a.paths, a.dx, a.dy, variables=tuple(a.variables), max_distance=a.mask, depth=depth, block=a.block, device=a.device,
                       out=out, elevation_edges=edges, elevation=a.elevation, intervals=a.intervals, **({"pooled": True} if a.pooled else {}))
    except ValueError as e:
        print("survey_volume: %s" % e, file=sys.stderr)
        return 1
    if a.intervals is not None:
        print("%d soundings -> %d x %d pixels, %d %s units: %s" % (r["x"].size, r["x_edges"].size - 1, r["y_edges"].size - 1,
                                                                  r["interval_edges"].size - 1, a.intervals["kind"],
                                                                  os.path.join(out, INTERVALS_AXES_FILE)))
        for name in a.variables:
            print("  %s %r" % (intervals_volume_path(out, name), tuple(r[name].shape)))
        return 0
    if "elevation_edges" in r:
        print("%d soundings -> %d x %d pixels, %d elevation cells %g .. %g m: %s" % (
            r["x"].size, r["x_edges"].size - 1, r["y_edges"].size - 1, r["elevation_edges"].size - 1, r["elevation_edges"][0],
            r["elevation_edges"][-1], os.path.join(out, AXES_FILE)))
    elif "elevation_level" in r:
        print("%d soundings -> %d x %d pixels at elevation %g m: %s" % (r["x"].size, r["x_edges"].size - 1, r["y_edges"].size - 1,
                                                                        r["elevation_level"], os.path.join(out, AXES_FILE)))
    else:
        print("%d soundings -> %d x %d pixels, %d depth cells: %s" % (r["x"].size, r["x_edges"].size - 1, r["y_edges"].size - 1,
                                                                      r["depth_edges"].size - 1, os.path.join(out, AXES_FILE)))
    for name in a.variables:
        print("  %s %r" % ((pooled_volume_path if a.pooled else volume_path)(out, name), tuple(r[name].shape)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
