#!/usr/bin/env python
"""Reference elevation slices for tests/test_elevation.py (build container only; needs the reference checkout that make_golden.py
imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_elevation_slices.py   ->  tests/golden/elevation_slices.npz

The IMPORTED reference's ``Inference2D.elevationSlice(elevation, values)`` (inversion/Inference2D.py:881-922) is called, unbound, on a
stub ``self`` that carries what the method reads: ``nPoints``, ``elevation`` and ``mesh = SimpleNamespace(z=RectilinearMesh1D(edges=
depth_edges), shape=values.shape)`` -- as written the method refers to a ``mesh.z`` that a line's 2-D mesh does not have, so it cannot be
reached through an ``Inference2D`` of its own.  ``values`` goes in as the reference lays it out, [n_depth, nPoints]; the fixture keeps
[nPoints, n_depth] and the outputs as [nPoints, levels] / [nPoints, intervals].

Two depth axes, each with 60 soundings over 40 m of relief (80 .. 120 m), one NaN value and one NaN surface elevation:
  resolve    the 440 cells of 0.5 m of the reference's Resolve posterior mesh (the ``y_edges`` make_line_products.py recorded from it);
  irregular  200 cells growing from 0.4 m to about 4 m, jittered, the edges multiples of 2^-8 m.
Levels: above every surface; two within the relief; mid-mesh; below every mesh; one EXACTLY on depth edge 37 of sounding 7 (z_s - E equals
the edge in every bit: side='right' gives cell 37); one exactly on sounding 7's surface (d = e[0]: the strict comparison gives NaN).
Intervals: the 12 cells of a regular 2.5 m axis, 60 .. 90 m, which the lowest surfaces cut (fewer than 8 depth cells each); intervals of
8 to 128 cells; of more than 128 cells, the whole mesh among them; one cut by every surface, one by every mesh bottom; one above
everything, one below everything and one reversed (all NaN).

Asserted: every case not meant to be all NaN has at least 40 % finite outputs, the others none; each of the three branches of the
pairwise sum (fewer than 8 terms, 8 to 128, more than 128) is taken by finite outputs; the plain numpy statement
(tests/elevation_reference.py) equals the reference in every output; and the number of finite interval outputs whose left-to-right sum
would differ in bits is above zero (printed).  The fixture holds data only.
"""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference   # noqa: E402

N = 60
ON_EDGE_SOUNDING, ON_EDGE_CELL = 7, 37
THIN_EDGES = (60.0, 90.0, 2.5)


def axes():
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(20261017))
    resolve = np.load(os.path.join(HERE, "line_products.npz"))["y_edges"].astype(np.float64)
    assert resolve.size == 441
    w = 0.4 * (10.0 ** (np.arange(200) / 199.0)) * rng.uniform(0.8, 1.25, 200)
    irregular = np.concatenate([[0.0], np.cumsum(np.maximum(np.round(w * 256.0), 1.0))]) / 256.0
    return rng, dict(resolve=resolve, irregular=irregular)


def cases(rng, e):
    import numpy as np
    n = e.size - 1
    z = 80.0 + 40.0 * rng.uniform(size=N)
    z[0], z[1], z[ON_EDGE_SOUNDING] = 80.0, 120.0, 98.0
    z[13] = np.nan
    v = rng.normal(size=(N, n))
    v[21, 150] = np.nan
    bottom = float(e[-1])
    on_edge = 98.0 - e[ON_EDGE_CELL]
    assert z[ON_EDGE_SOUNDING] - on_edge == e[ON_EDGE_CELL]
    levels = [(130.0, True), (96.0, False), (85.5 + 1.0 / 64.0, False), (100.0 - 0.5 * bottom, False), (75.0 - bottom, True),
              (on_edge, False), (98.0, False)]
    thin = np.arange(THIN_EDGES[0], THIN_EDGES[1] + 0.5 * THIN_EDGES[2], THIN_EDGES[2])
    ivals = [(a, b, False) for a, b in zip(thin[:-1], thin[1:])]
    ivals += [(40.0, 70.0, False), (55.0, 58.7, False), (61.3, 77.1, False),                       # 8 .. 128 cells
              (-20.0, 75.0, False), (-60.0, 79.5, False), (-500.0, 500.0, False),                   # more than 128; the whole mesh
              (70.0, 125.0, False),                                                                 # cut by every surface
              (80.0 - bottom - 30.0, 80.0 - bottom + 30.0, False),                                  # cut by every mesh bottom
              (125.0, 140.0, True), (70.0 - bottom - 30.0, 75.0 - bottom, True), (70.0, 40.0, True)]   # above, below, reversed
    return z, v, levels, ivals


def main():
    import numpy as np
    import_reference()
    from geobipy import RectilinearMesh1D
    from geobipy.src.inversion.Inference2D import Inference2D
    import elevation_reference as er

    rng, ax = axes()
    out = {"axes": np.array(sorted(ax))}
    branches = set()
    differ = finite_means = 0
    for name in sorted(ax):
        e = ax[name]
        z, v, levels, ivals = cases(rng, e)
        vt = np.ascontiguousarray(v.T)                                       # [n_depth, nPoints], the reference's layout
        stub = types.SimpleNamespace(nPoints=N, elevation=z, mesh=types.SimpleNamespace(z=RectilinearMesh1D(edges=e.copy()), shape=vt.shape))

        def ref(elevation):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                                # (the mean of an empty slice: the reversed interval)
                return np.asarray(Inference2D.elevationSlice(stub, elevation, vt), dtype=np.float64)

        lv = np.array([l for l, _ in levels])
        lo, hi = np.array([a for a, _, _ in ivals]), np.array([b for _, b, _ in ivals])
        level_out = np.stack([ref(np.float64(l)) for l in lv], axis=1)      # [N, levels]
        interval_out = np.stack([ref(np.array([a, b])) for a, b in zip(lo, hi)], axis=1)
        for k, (_, nan_all) in enumerate(levels):
            share = np.isfinite(level_out[:, k]).mean()
            assert (share == 0.0) if nan_all else (share >= 0.4), (name, "level", k, share)
        for k, (_, _, nan_all) in enumerate(ivals):
            share = np.isfinite(interval_out[:, k]).mean()
            assert (share == 0.0) if nan_all else (share >= 0.4), (name, "interval", k, share)
        # the edge cases are what they are meant to be
        assert level_out[ON_EDGE_SOUNDING, 5] == v[ON_EDGE_SOUNDING, ON_EDGE_CELL] and np.isnan(level_out[ON_EDGE_SOUNDING, 6])
        assert np.isnan(level_out[13]).all() and np.isnan(interval_out[13]).all()
        assert np.isnan(interval_out[21]).any() and np.isfinite(interval_out[21]).any()
        # the branches of the sum the finite outputs took
        with np.errstate(invalid="ignore"):
            d0, d1 = z[:, None] - lo[None, :], z[:, None] - hi[None, :]
            count = np.where((d1 < e[-1]) & (d0 > e[0]), er.cell(e, d0) - er.cell(e, d1) + 1, 0)
        fin = np.isfinite(interval_out)
        branches |= {("<8", "8..128", ">128")[int(c >= 8) + int(c > 128)] for c in count[fin]}
        assert (count[fin] > 0).all() and (count[:, :12][fin[:, :12]] < 8).all()
        # the plain statement, and the order it must not have
        same = lambda a, b: bool(np.all((a == b) | ((a != a) & (b != b))))
        assert same(er.at_levels(v, z, e, lv), level_out), name
        assert same(er.over_intervals(v, z, e, lo, hi), interval_out), name
        l2r = er.over_intervals(v, z, e, lo, hi, total=er.left_to_right_sum)
        differ += int((fin & (l2r != interval_out)).sum())
        finite_means += int(fin.sum())
        out.update({name + "_depth_edges": e, name + "_surface": z, name + "_values": v, name + "_levels": lv,
                    name + "_level_out": level_out, name + "_level_all_nan": np.array([f for _, f in levels]),
                    name + "_lo": lo, name + "_hi": hi, name + "_interval_out": interval_out,
                    name + "_interval_all_nan": np.array([f for _, _, f in ivals])})
        print("%-9s %3d cells to %.4g m: levels finite %s" % (name, e.size - 1, e[-1], np.isfinite(level_out).sum(axis=0).tolist()))
        print("          intervals finite %s" % np.isfinite(interval_out).sum(axis=0).tolist())
        print("          cells per interval (median of the finite) %s" % [
            int(np.median(count[fin[:, k], k])) if fin[:, k].any() else 0 for k in range(lo.size)])
    assert branches == {"<8", "8..128", ">128"}, branches
    print("finite interval outputs: %d; a left-to-right sum differs in bits in %d of them" % (finite_means, differ))
    assert differ > 0
    out.update(on_edge_sounding=np.int64(ON_EDGE_SOUNDING), on_edge_cell=np.int64(ON_EDGE_CELL), on_edge_level=np.int64(5),
               on_surface_level=np.int64(6), thin_edges=np.arange(THIN_EDGES[0], THIN_EDGES[1] + 0.5 * THIN_EDGES[2], THIN_EDGES[2]),
               thin_intervals=np.int64(12))
    path = os.path.join(HERE, "elevation_slices.npz")
    np.savez_compressed(path, **out)
    print("wrote elevation_slices.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
