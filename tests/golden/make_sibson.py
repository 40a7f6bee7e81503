#!/usr/bin/env python
"""Reference discrete Sibson gridding for tests/test_survey_volume.py (build container only; needs the reference checkout
that make_golden.py imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sibson.py   ->  tests/golden/sibson.npz

The IMPORTED reference's ``interpolation.sibson(x, y, values[:, c], x_edges, y_edges, max_distance=...)`` (base/interpolation.py:24-89)
is recorded column by column.  Its ``numba.jit`` is the identity here (make_golden.import_reference) and its ``numba_kdtree.KDTree`` is
replaced by an adapter over ``scipy.spatial.cKDTree`` whose ``query(q, k=1)`` returns (distance array, index array, None).  Per case
the recorder also keeps ``index`` and ``D`` -- the answers the adapter gave to the reference's own queries, pixel by pixel -- and ``n``,
the reference's own counter: the module's ``zeros``, from which ``__sibson_2d_inner`` allocates ``c`` and ``n``, is wrapped to capture
the int32 array, which is read after the call.  So the plan is pinned apart from the sums.

Cases:
  cloud     60 soundings at random over 17 x 12 pixels, C = 3;
  lines     four jittered flight lines, a gap in one, dx = 16, dy = 32, one sounding exactly on a grid node (D = 0 there), one sounding
            outside the grid, one NaN value, no mask, C = 2;
  masked    the same with a finite max_distance that masks part of the grid;
  single    one sounding on 9 x 7;
  five      5 soundings on 40 x 36 (long cover lists);
  centred   the cloud on the grid of the reference's ``Point.centred_grid_nodes`` over its bounds (the edges are recorded from it).

Asserted, so that no tie and no rounding edge enters the comparison:
  * at every pixel the squared distances to the nearest and the second-nearest sounding differ by more than 1e-9 relative;
  * at every pixel the nearest distance is farther than 1e-9 from every integer, or its square is exactly a perfect square (the on-node
    sounding gives exact integers along its row and column: those are wanted).
The smallest gaps met are printed.  The fixture holds data only.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference   # noqa: E402


def cases():
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(20261016))
    out = {}
    xe, ye = 1000.0 + 25.0 * np.arange(18), 500.0 + 40.0 * np.arange(13)
    cx, cy = rng.uniform(xe[0], xe[-1], 60), rng.uniform(ye[0], ye[-1], 60)
    cv = rng.normal(size=(60, 3))
    out["cloud"] = dict(x=cx, y=cy, values=cv, x_edges=xe, y_edges=ye, max_distance=np.inf)
    # four lines along x, 64 m apart in y (2 pixels), soundings every ~20 m; a gap in line 2
    xe, ye = 4000.0 + 16.0 * np.arange(27), 9000.0 + 32.0 * np.arange(15)
    lx, ly = [], []
    for k in range(4):
        t = np.arange(4010.0, 4410.0, 20.0)
        if k == 2:
            t = t[(t < 4130.0) | (t > 4290.0)]
        lx.append(t + rng.uniform(-3.0, 3.0, t.size))
        ly.append(9070.0 + 96.0 * k + rng.uniform(-5.0, 5.0, t.size))
    lx, ly = np.concatenate(lx), np.concatenate(ly)
    lx, ly = np.r_[lx, 4000.0 + 16.0 * 11, 4500.0], np.r_[ly, 9000.0 + 32.0 * 6, 9100.0]      # on node (11, 6); outside the grid
    lv = rng.normal(size=(lx.size, 2))
    lv[17, 1] = np.nan
    out["lines"] = dict(x=lx, y=ly, values=lv, x_edges=xe, y_edges=ye, max_distance=np.inf)
    out["masked"] = dict(x=lx, y=ly, values=lv, x_edges=xe, y_edges=ye, max_distance=16.0 * 32.0 * 5.0)
    out["single"] = dict(x=np.array([33.7]), y=np.array([-12.2]), values=np.array([[2.5]]), x_edges=10.0 * np.arange(10),
                         y_edges=-40.0 + 8.0 * np.arange(8), max_distance=np.inf)
    out["five"] = dict(x=rng.uniform(0.0, 400.0, 5), y=rng.uniform(0.0, 180.0, 5), values=rng.normal(size=(5, 2)),
                       x_edges=10.0 * np.arange(41), y_edges=5.0 * np.arange(37), max_distance=np.inf)
    out["centred"] = dict(x=cx, y=cy, values=cv[:, :1], spacing=(30.0, 45.0), max_distance=np.inf)
    return out


def main():
    import numpy as np
    from scipy.spatial import cKDTree
    import_reference()
    from geobipy.src.base import interpolation
    from geobipy.src.classes.pointcloud.Point import Point

    asked = []

    class Tree:
        def __init__(self, points, leafsize=16):
            self.points = np.array(points, dtype=np.float64)
            self.tree = cKDTree(self.points, leafsize=leafsize)

        def query(self, q, k=1):
            d, ix = self.tree.query(np.asarray(q, dtype=np.float64)[None, :], k=1)
            asked.append((self.points, tuple(q), float(d[0]), int(ix[0])))
            return np.atleast_1d(d), np.atleast_1d(ix), None

    made = []
    np_zeros = interpolation.zeros

    def zeros(*a, **k):
        z = np_zeros(*a, **k)
        made.append(z)
        return z

    interpolation.KDTree = Tree
    interpolation.zeros = zeros

    out = {}
    gap2, gapi = np.inf, np.inf
    for name, c in cases().items():
        if "spacing" in c:
            b = np.asarray([np.nanmin(c["x"]), np.nanmax(c["x"]), np.nanmin(c["y"]), np.nanmax(c["y"])])
            c["x_edges"] = np.asarray(Point.centred_grid_nodes(None, b[:2], c["spacing"][0]), dtype=np.float64)
            c["y_edges"] = np.asarray(Point.centred_grid_nodes(None, b[2:], c["spacing"][1]), dtype=np.float64)
            out[name + "_bounds"], out[name + "_spacing"] = b, np.asarray(c["spacing"])
        nx, ny = c["x_edges"].size - 1, c["y_edges"].size - 1
        cols = []
        for col in range(c["values"].shape[1]):
            del asked[:], made[:]
            r = interpolation.sibson(c["x"].copy(), c["y"].copy(), c["values"][:, col].copy(), c["x_edges"].copy(), c["y_edges"].copy(),
                                     max_distance=c["max_distance"])
            cols.append(np.asarray(r, dtype=np.float64))
            n = [z for z in made if z.dtype == np.int32]
            assert len(n) == 1 and n[0].shape == (ny, nx) and len(asked) == nx * ny
            index = np.array([a[3] for a in asked], dtype=np.int32).reshape(ny, nx)
            D = np.array([int(np.int32(np.ceil(a[2]))) for a in asked], dtype=np.int32).reshape(ny, nx)
            assert [a[1] for a in asked] == [(j, i) for i in range(ny) for j in range(nx)]
            if col:
                assert np.array_equal(index, out[name + "_index"]) and np.array_equal(D, out[name + "_D"]) and np.array_equal(n[0], out[name + "_n"])
            out[name + "_index"], out[name + "_D"], out[name + "_n"] = index, D, n[0].copy()
        # the conditions on the geometry
        pts = asked[0][0]
        for i in range(ny):
            for j in range(nx):
                d2 = np.sort((j - pts[:, 0]) ** 2 + (i - pts[:, 1]) ** 2)
                if d2.size > 1:
                    g = (d2[1] - d2[0]) / d2[1]
                    assert g > 1e-9, (name, i, j, g)
                    gap2 = min(gap2, g)
                r = np.sqrt(d2[0])
                off = abs(r - np.rint(r))
                exact = float(np.rint(r)) ** 2 == d2[0]
                assert off > 1e-9 or exact, (name, i, j, r)
                if not exact:
                    gapi = min(gapi, off)
        out[name + "_out"] = np.stack(cols)
        for k in ("x", "y", "values", "x_edges", "y_edges"):
            out[name + "_" + k] = np.asarray(c[k], dtype=np.float64)
        out[name + "_max_distance"] = np.float64(c["max_distance"])
        o = out[name + "_out"]
        print("%-8s N %3d grid %2d x %2d C %d  D 0..%d (zeros %d)  n min/median/max %d/%d/%d  NaN pixels %d" % (
            name, c["x"].size, nx, ny, o.shape[0], out[name + "_D"].max(), int((out[name + "_D"] == 0).sum()), out[name + "_n"].min(),
            int(np.median(out[name + "_n"])), out[name + "_n"].max(), int(np.isnan(o).sum())))
    out["cases"] = np.array(sorted(cases()))
    print("asserted: nearest / second-nearest squared distances differ by > 1e-9 relative at every pixel (smallest gap %.3g);" % gap2)
    print("asserted: every nearest distance is > 1e-9 from an integer or exactly an integer (smallest distance to one %.3g)" % gapi)
    np.savez_compressed(os.path.join(HERE, "sibson.npz"), **out)
    print("wrote sibson.npz", os.path.getsize(os.path.join(HERE, "sibson.npz")), "bytes")


if __name__ == "__main__":
    main()
