#!/usr/bin/env python
"""Reference values of the interval (unit) products of the eight hit maps of line_products.npz (build container only; needs
/root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_interval_products.py   ->  tests/golden/interval_products.npz

The counts are read from line_products.npz, not duplicated.  Three cases, each for all eight maps:

  partition  (A) one depth partition for every map.  The cells of each interval come from the IMPORTED reference's own rule,
             ``scipy.stats.binned_statistic(mesh.y.centres, counts, bins=edges, statistic='sum')`` -- what its
             ``RectilinearMesh2D.intervalStatistic`` calls (mesh/RectilinearMesh2D.py:507-558; the method itself trims the intervals
             against the wrong axis and is not used) -- and the marginals are asserted equal to
             ``Histogram[:, lo:hi].marginalize(axis=1).counts`` (statistics/Histogram.py:60-64, 236-260).
  elevation  (B) one elevation axis under a different surface per map: the same binning of surface - centre.
  pairs      (B) one overlapping set of depth pairs through the reference's ``Inference2D._z_slice`` (inversion/Inference2D.py:828-843).

The statistics are those of the reference's 2-D ``Histogram`` over (the posterior's value axis x an interval axis) filled with the
marginals, along axis 0 -- the functions the per-cell products are pinned to (make_line_products.py, make_class_probability.py):
``mean``, ``mode``, ``percentile`` for the five percentiles of line_products.npz, ``credible_range(90, log=10)`` and
``compute_probability(MvNormal(...), log=10, axis=0)`` for the class sets of make_class_probability.py.  (The reference's statistics
on a 1-D marginal Histogram raise; its 2-D ones do not depend on the second axis.)

The inputs hold: an edge exactly on a cell centre and one on a cell edge, the closed last edge (a centre equal to edges[-1]), an interval
above the surface and one below the mesh, a one-cell interval, and an interval of map 6 whose sum exceeds 2^31 -- all asserted below.

Where a cumulative share of a marginal falls EXACTLY on a percentile (100 cum == p total, in integers) the reference's cell is decided
by rounding (make_line_products.py: ``_nudge_ties``); a marginal cannot be nudged, so those (map, interval) entries are MARKED
(``ties_<case>``) and only the percentile / credible comparisons skip them.  The free edges are drawn from a seed, the first seed taken
whose marked entries are at most 10 % of the entries with counts and whose entries without cells are at most a quarter of all; both
are asserted on the recorded values.  The fixture holds data only.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import import_reference   # noqa: E402
from make_class_probability import class_sets, posterior   # noqa: E402

SURFACES = (101.3, 99.75, 120.0, 87.25, 95.5, 110.0, 102.0, 100.0)      # one per map (m)
ELEVATION_EDGES = tuple(range(-140, 131, 30))
MAX_MARKED, MAX_EMPTY = 0.10, 0.25


def candidate(seed):
    """(partition edges, pairs) of ``seed``: the fixed edges carry the cases listed above, the free ones are multiples of 0.5 m."""
    import numpy as np
    rng = np.random.default_rng(seed)
    half = lambda lo, hi: 0.5 * rng.integers(int(2 * lo), int(2 * hi))          # noqa: E731
    a1, a2 = half(8, 15), half(16, 40)
    a3, a4 = half(70, 88), half(89, 110)
    # -3 .. -1: above the surface; 59.25: a cell centre; 62.5, 63: cell edges, one cell between; 114.5 .. 159.5: 90 cells (map 6 > 2^31);
    # 206.25: a cell centre, the closed last edge
    partition = np.array([-3.0, -1.0, a1, a2, 59.25, 62.5, 63.0, a3, a4, 114.5, 159.5, 206.25])
    b1, b2 = half(3, 12), half(20, 40)
    pairs = np.array([[0.0, b1], [0.5 * b1, b2], [b2, 75.0], [74.9, 75.1], [12.3, 12.4], [100.0, 219.9], [half(150, 200), 60.0]])
    return partition, pairs


def marks(marg, percentiles):
    """[maps, M] bool: a cumulative share of the marginal [maps, nv, M] (int64) falls exactly on a percentile."""
    import numpy as np
    cum = np.cumsum(marg, axis=1)
    tot = marg.sum(axis=1)
    hit = np.zeros(tot.shape, dtype=bool)
    for p in percentiles:
        assert float(p) == int(p)
        hit |= np.any(100 * cum == int(p) * tot[:, None, :], axis=1) & (tot > 0)
    return hit


def census(counts, d_edges, partition, pairs, percentiles):
    """(marked, with counts, without cells, all) over the three cases, by the package's own range builders (the search only)."""
    import numpy as np
    from geobipy_amd import intervals as iv
    P = np.zeros(counts.shape[:2] + (counts.shape[2] + 1,), dtype=np.int64)
    P[:, :, 1:] = np.cumsum(counts.astype(np.int64), axis=2)
    n = len(counts)
    sets = [iv.Ranges(*(np.broadcast_to(a, (n, a.size)) for a in iv.depth_ranges(d_edges, partition))),
            iv.elevation_ranges(SURFACES, d_edges, ELEVATION_EDGES),
            iv.Ranges(*(np.broadcast_to(a, (n, a.size)) for a in iv.depth_pairs(d_edges, pairs)))]
    marked = full = empty = total = 0
    for r in sets:
        marg = np.stack([P[b][:, r.hi[b]] - P[b][:, r.lo[b]] for b in range(n)])
        marked += int(marks(marg, percentiles).sum())
        full += int((marg.sum(axis=1) > 0).sum())
        empty += int((r.n_cells == 0).sum())
        total += r.n_cells.size
    return marked, full, empty, total


def main():
    import numpy as np
    from scipy.stats import binned_statistic, norm
    import_reference()
    from geobipy import Histogram, RectilinearMesh1D, RectilinearMesh2D
    from geobipy.src.classes.statistics import baseDistribution as bd
    from geobipy.src.classes.statistics.MvNormalDistribution import MvNormal
    from geobipy.src.inversion.Inference2D import Inference2D

    def _init(self, prng=None):                                   # (make_class_probability.py: the probabilities draw no random numbers)
        self.prng = np.random.Generator(np.random.PCG64DXSM(0)) if prng is None else prng
    bd.baseDistribution.__init__ = _init

    lp = dict(np.load(os.path.join(HERE, "line_products.npz")))
    counts = lp["counts"]                                         # [8, n_value, n_depth] int32
    n, nv, nz = counts.shape
    percentiles = tuple(float(p) for p in lp["percentiles"])
    credible = float(lp["credible"])
    h = posterior()
    mesh = h.mesh
    assert np.array_equal(np.asarray(mesh.x.edges, dtype=np.float64), lp["x_edges"])
    assert np.array_equal(np.asarray(mesh.y.edges, dtype=np.float64), lp["y_edges"])
    assert float(np.asarray(mesh.x.relative_to).ravel()[0]) == float(lp["relative_to"])
    d_edges = lp["y_edges"]
    centres = np.asarray(mesh.y.centres, dtype=np.float64)
    assert centres.tobytes() == (0.5 * (d_edges[1:] + d_edges[:-1])).tobytes()          # the package's depth_centres, bit for bit
    xc = np.log10(np.asarray(mesh.centres(axis=0), dtype=np.float64))
    sets = class_sets(float(xc.min()), float(xc.max()))
    xc = xc.reshape(nv, -1)[:, 0]                                 # (one relative_to: the centres do not change along depth)

    seed = 0
    while True:
        partition, pairs = candidate(seed)
        marked, full, empty, total = census(counts, d_edges, partition, pairs, percentiles)
        if marked <= MAX_MARKED * full and empty <= MAX_EMPTY * total:
            break
        seed += 1
        assert seed < 10000
    print("seed", seed, "marked", marked, "of", full, "with counts;", empty, "of", total, "without cells")
    print("partition", partition, "pairs", pairs.tolist())

    def cells_of(binnumber, M):
        """lo, hi [M] of the cells binned_statistic put into bins 1 .. M (contiguous along depth, asserted)."""
        lo, hi = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        for m in range(M):
            j = np.flatnonzero(binnumber == m + 1)
            if j.size:
                assert np.array_equal(j, np.arange(j[0], j[-1] + 1))
                lo[m], hi[m] = j[0], j[-1] + 1
        return lo, hi

    def reference_marginal(c, lo, hi):
        """[nv, M] int64 through Histogram[:, lo:hi].marginalize(axis=1); zeros where there are no cells."""
        h.values = c.astype(np.int32)
        out = np.zeros((nv, lo.size), dtype=np.int64)
        for m in range(lo.size):
            if hi[m] > lo[m]:
                v = np.asarray(h[:, int(lo[m]):int(hi[m])].marginalize(axis=1).counts)
                assert v.dtype.kind in "if" and np.array_equal(v, np.round(v)) and np.abs(v).max() < 2.0 ** 53     # (exact either way)
                out[:, m] = v.astype(np.int64)
        return out

    z_axis = types.SimpleNamespace(mesh=types.SimpleNamespace(z=RectilinearMesh1D(edges=d_edges)))
    cases = {}
    for case in ("partition", "elevation", "pairs"):
        lo_all, hi_all, marg_all = [], [], []
        for b, c in enumerate(counts):
            if case == "pairs":
                sl = [Inference2D._z_slice(z_axis, depth=np.array(p, dtype=np.float64)) for p in pairs]
                lo, hi = np.array([s.start for s in sl], dtype=np.int32), np.array([s.stop for s in sl], dtype=np.int32)
                marg = reference_marginal(c, lo, hi)
            else:
                x, edges = (centres, partition) if case == "partition" else (SURFACES[b] - centres, np.asarray(ELEVATION_EDGES, dtype=np.float64))
                r = binned_statistic(x, c, bins=edges, statistic="sum")
                lo, hi = cells_of(r.binnumber, edges.size - 1)
                marg = np.asarray(r.statistic)
                assert marg.shape == (nv, edges.size - 1) and np.array_equal(marg, np.round(marg)) and marg.max() < 2.0 ** 53
                marg = marg.astype(np.int64)
                assert np.array_equal(marg, reference_marginal(c, lo, hi)), (case, b)
            lo_all.append(lo), hi_all.append(hi), marg_all.append(marg)
        cases[case] = (np.stack(lo_all), np.stack(hi_all), np.stack(marg_all))

    # what the inputs hold
    lo, hi, marg = cases["partition"]
    assert 59.25 in centres and 62.5 in d_edges and partition[-1] in centres
    assert hi[0, -1] - 1 == np.flatnonzero(centres == partition[-1])[0]                  # the closed last edge took its cell
    assert (hi - lo)[0, 0] == 0 and (hi - lo)[0, 5] == 1                                # above the surface; one cell
    assert marg[6].sum(axis=0).max() > 2 ** 31
    elo, ehi, _ = cases["elevation"]
    assert any(np.any(SURFACES[b] - centres == e) for b in range(n) for e in ELEVATION_EDGES)          # an edge on a cell centre
    assert ((ehi - elo)[:, -1] == 0).any() and ((ehi - elo)[2, 0] == 0) and SURFACES[2] - ELEVATION_EDGES[1] > d_edges[-1]   # above; below
    plo, phi, _ = cases["pairs"]
    assert np.any((plo[0][:, None] < phi[0][None, :]) & (plo[0][None, :] < phi[0][:, None]) & ~np.eye(plo.shape[1], dtype=bool))   # overlap

    out = dict(percentiles=np.asarray(percentiles), credible=credible, seed=seed, partition_edges=partition, pairs=pairs,
               elevation_edges=np.asarray(ELEVATION_EDGES, dtype=np.float64), surfaces=np.asarray(SURFACES), sets=np.array(sorted(sets)))
    for name, (means, scales) in sorted(sets.items()):
        out["means_" + name], out["scales_" + name] = np.asarray(means, dtype=np.float64), np.asarray(scales, dtype=np.float64)
    marked = full = empty = total = 0
    for case, (lo, hi, marg) in cases.items():
        M = lo.shape[1]
        h2 = Histogram(mesh=RectilinearMesh2D(x=mesh.x, y=RectilinearMesh1D(edges=np.arange(M + 1, dtype=np.float64))))
        rec = {k: [] for k in ("mean", "mode", "percentiles", "credible_range")}
        cls = {name: ([], [], []) for name in sets}
        for b in range(n):
            h2.values = marg[b]
            assert np.array_equal(np.asarray(h2.counts), marg[b])
            rec["mean"].append(np.log10(np.asarray(h2.mean(axis=0).values, dtype=np.float64)))
            rec["mode"].append(np.log10(np.asarray(h2.mode(axis=0).values, dtype=np.float64)))
            rec["percentiles"].append(np.stack([np.log10(np.asarray(h2.percentile(percent=q, axis=0).values, dtype=np.float64))
                                                for q in percentiles]))
            rec["credible_range"].append(np.asarray(h2.credible_range(percent=credible, log=10, axis=0), dtype=np.float64))
            for name, (means, scales) in sets.items():
                mu, sd = np.asarray(means, dtype=np.float64), np.asarray(scales, dtype=np.float64)
                phi = np.stack([norm.pdf(xc, loc=m_, scale=s_) for m_, s_ in zip(mu, sd)])       # [K, n_value]
                big = (marg[b][None, :, :] * phi[:, :, None]).reshape(-1, M).max(axis=0)
                assert np.all((big == 0.0) | (big >= np.finfo(np.float64).tiny)), (case, name)   # (no subnormal rounding in the comparison)
                p = np.asarray(h2.compute_probability(MvNormal(mean=mu, variance=sd), log=10, axis=0, track=False), dtype=np.float64)
                assert p.shape == (mu.size, M), p.shape
                j = np.argmax(p, axis=0)
                cls[name][0].append(p), cls[name][1].append(j.astype(np.int32))
                cls[name][2].append(np.take_along_axis(p, j[None], axis=0)[0])
        ties = marks(marg, percentiles)
        out.update({"lo_" + case: lo, "hi_" + case: hi, "marginals_" + case: marg, "ties_" + case: ties})
        out.update({"ref_%s_%s" % (k, case): np.stack(v) for k, v in rec.items()})
        for name, (p, j, bp) in cls.items():
            out.update({"prob_%s_%s" % (name, case): np.stack(p), "best_%s_%s" % (name, case): np.stack(j),
                        "best_p_%s_%s" % (name, case): np.stack(bp)})
        marked += int(ties.sum())
        full += int((marg.sum(axis=1) > 0).sum())
        empty += int((hi - lo == 0).sum())
        total += lo.size
        print(case, "M", M, "marked", int(ties.sum()), "with counts", int((marg.sum(axis=1) > 0).sum()), "without cells", int((hi - lo == 0).sum()))
    assert marked <= MAX_MARKED * full, (marked, full)
    assert empty <= MAX_EMPTY * total, (empty, total)
    out["census"] = np.array([marked, full, empty, total])
    np.savez_compressed(os.path.join(HERE, "interval_products.npz"), **out)
    print("wrote interval_products.npz", os.path.getsize(os.path.join(HERE, "interval_products.npz")), "bytes;", marked, "of", full, "marked")


if __name__ == "__main__":
    main()
