#!/usr/bin/env python
"""Reference values of the posterior line products (build container only; needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_line_products.py   ->  tests/golden/line_products.npz

The posterior mesh is built as make_hitmap_stats.py builds it: the IMPORTED reference initialises an ``Inference1D`` on one Resolve
sounding, and ``model.values.posterior`` is the ``Histogram`` over a ``RectilinearMesh2D`` of 250 value cells (log10, relative to the
prior mean) by 440 depth cells.  Eight hit maps are assigned to its counts in turn -- layered posteriors like the chains leave, one whose
cumulative shares fall EXACTLY on a quantile (elsewhere no share does: ``_nudge_ties``), one with argmax ties, one with empty columns
(and an empty map), one with counts whose sum c ln c needs fp64 -- and the reference's own per-sounding products are recorded (all along the value axis):
``Histogram.mode``, ``Histogram.percentile`` (statistics/Histogram.py:308-401 -> mesh/Mesh.py:138-215), ``credible_range(90, log=10)``
(Histogram.py:113-127 -> Mesh.py:58-78), ``entropy`` (bits; Histogram.py:129-148 over ``Histogram.pdf``, :34-41) and ``opacity(90,
log=10)`` (Histogram.py:330-354, 509-542).  An interface-depth histogram per sounding gives ``Histogram.pdf`` over the 1-D depth mesh,
and the eight of them stacked, over the line's 2-D (sounding index, depth) mesh, the line's interface probability.

The line-level opacity and the DOI are the formulas of the reference applied to its own per-sounding outputs (a 3-D reference
Histogram over the line is not needed for them): the transparency of statistics/Histogram.py:509-542 -- the credible range normalised
by its nanmin / nanmax over ALL soundings and depth cells, NaN -> 1 -- and the walk of inversion/Inference2D.py:493-535 (from the
deepest cell up while the opacity is below 0.67, stopping at cell 0).  The fixture holds data only: counts, edges, the outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, SUP, import_reference   # noqa: E402

PERCENTILES = (5.0, 16.0, 50.0, 84.0, 95.0)
CREDIBLE = 90.0
DOI = 67.0


def _maps(nx, ny, rng):
    import numpy as np
    maps = []
    for kind in range(8):
        c = np.zeros((nx, ny), dtype=np.int32)                   # [value, depth] -- the device's layout
        if kind in (0, 1, 2):                                    # layered posteriors: a few layers, many, a smear
            for _ in range((12, 60, 200)[kind]):
                v = rng.integers(0, nx)
                lo, hi = np.sort(rng.integers(0, ny, 2))
                c[v, lo:hi + 1] += rng.integers(1, 900)
        elif kind == 3:                                          # 20 samples per column: the 5 / 50 / 95 % points fall ON a cumulative share
            for z in range(ny):
                vs = np.sort(rng.choice(nx, 4, replace=False))
                c[vs, z] = (1, 9, 9, 1)
        elif kind == 4:                                          # argmax ties: two or three equal maxima per column
            for z in range(ny):
                vs = rng.choice(nx, 3, replace=False)
                c[vs, z] = (40, 40, 40 if z % 2 else 17)
                c[rng.integers(0, nx), z] += rng.integers(0, 3)
        elif kind == 5:                                          # empty columns among full ones
            for z in range(0, ny, 3):
                c[rng.integers(0, nx, 5), z] += rng.integers(1, 50, 5).astype(np.int32)
        elif kind == 6:                                          # counts near 2^31 / 250: sum c ln c ~ 1e11 needs fp64
            for z in range(ny):
                lo = rng.integers(0, nx - 40)
                c[lo:lo + 40, z] = rng.integers(1 << 22, 1 << 23, 40)
        elif kind == 7:                                          # an empty map (a sounding that never ran)
            pass
        if kind != 3:
            _nudge_ties(c, rng)
        maps.append(c)
    return maps


def _nudge_ties(c, rng):
    """Add a count to an empty cell of every column whose cumulative share falls EXACTLY on one of the percentiles (100 cum == p total,
    in integers), until none does.  The reference's cell there is decided by rounding (Histogram.percentile cumulates the pmf c / sum c,
    mesh/Mesh.py:198-210, so its share lands an ulp to either side); the deliberate ties of map 3 are kept -- its rounding and the exact
    rule agree on them."""
    import numpy as np
    for z in range(c.shape[1]):
        while True:
            col = c[:, z].astype(np.int64)
            tot, cum = col.sum(), np.cumsum(col)
            if tot == 0 or not any(np.any(100 * cum == int(p) * tot) for p in PERCENTILES):   # (the credible bounds among them)
                break
            c[rng.choice(np.flatnonzero(col == 0)), z] += 1


def main():
    import numpy as np
    import_reference()
    from geobipy import FdemData, Histogram, Inference1D, RectilinearMesh1D, RectilinearMesh2D, get_prng
    from geobipy.src.inversion import user_parameters as up

    opt_file = REF + "/documentation_source/source/supplementary/options_files/resolve_options"
    options = up.user_parameters.read(opt_file, data_directory=SUP)
    options["system_filename"] = SUP + "/resolve.stm"
    options["n_markov_chains"] = 100
    options["save_hdf5"] = False
    options["interactive_plot"] = True
    options["update_plot_every"] = 100000
    data = FdemData.read_csv(SUP + "/resolve_glacial.csv", system=options["system_filename"])
    dp = data.datapoint(30)
    inf = Inference1D(prng=get_prng(seed=options["seed"] if "seed" in options else 1), **options)
    inf.initialize(dp)
    h = inf.model.values.posterior
    mesh = h.mesh
    x_edges = np.asarray(mesh.x.edges, dtype=np.float64)          # value axis (relative to the prior mean, log10)
    y_edges = np.asarray(mesh.y.edges, dtype=np.float64)          # depth
    rel_to = float(np.asarray(mesh.x.relative_to).ravel()[0])
    nx, ny = mesh.x.nCells.item(), mesh.y.nCells.item()
    assert tuple(h.counts.shape) == (nx, ny), h.counts.shape      # value axis 0
    print("value cells", nx, "depth cells", ny, "relative_to", rel_to, "x log", mesh.x.log)

    rng = np.random.default_rng(23)
    maps = _maps(nx, ny, rng)
    rec = {k: [] for k in ("mode", "percentiles", "credible_range", "entropy", "opacity")}
    for c in maps:
        h.values = c.astype(np.int32)
        rec["mode"].append(np.log10(np.asarray(h.mode(axis=0).values, dtype=np.float64)))
        rec["percentiles"].append(np.stack([np.log10(np.asarray(h.percentile(percent=q, axis=0).values, dtype=np.float64))
                                            for q in PERCENTILES]))
        rec["credible_range"].append(np.asarray(h.credible_range(percent=CREDIBLE, log=10, axis=0), dtype=np.float64))
        rec["entropy"].append(np.asarray(h.entropy(axis=0).values, dtype=np.float64))
        rec["opacity"].append(np.asarray(h.opacity(percent=CREDIBLE, log=10, axis=0).values, dtype=np.float64))
    out = dict(x_edges=x_edges, y_edges=y_edges, relative_to=rel_to, counts=np.stack(maps), percentiles=np.asarray(PERCENTILES),
               credible=CREDIBLE, doi_percent=DOI)
    for k, v in rec.items():
        out["ref_" + k] = np.stack(v)

    # interface-depth posteriors: one per sounding, 1-D over the depth edges; and the line's, 2-D over (sounding index, depth)
    iface = np.zeros((len(maps), ny), dtype=np.int32)
    for b in range(len(maps) - 1):                                # (the last sounding: empty)
        iface[b, rng.integers(0, ny, 30)] += rng.integers(1, 500, 30).astype(np.int32)
    pdf1 = []
    for b in range(len(maps)):
        hi = Histogram(mesh=RectilinearMesh1D(edges=y_edges))
        hi.values = iface[b]
        pdf1.append(np.asarray(hi.pdf.values, dtype=np.float64))
    line_x_edges = np.arange(len(maps) + 1, dtype=np.float64) - 0.5
    h2 = Histogram(mesh=RectilinearMesh2D(x_edges=line_x_edges, y_edges=y_edges))
    h2.values = iface
    out.update(interface_counts=iface, line_x_edges=line_x_edges, ref_interface_pdf=np.stack(pdf1),
               ref_line_interface_pdf=np.asarray(h2.pdf.values, dtype=np.float64))

    # line level: Histogram.transparency (statistics/Histogram.py:531-540) over the whole line, then the DOI walk (Inference2D.py:508-518)
    r = out["ref_credible_range"]
    mn, mx = np.nanmin(r), np.nanmax(r)
    t = (r - mn) / (mx - mn) if mx - mn > 0.0 else r - mn
    t[np.isnan(t)] = 1.0
    op = 1.0 - t
    doi_idx = np.empty(len(maps), dtype=np.int64)
    for i in range(len(maps)):
        j = ny - 1
        while op[i, j] < 0.01 * DOI and j >= 1:
            j -= 1
        doi_idx[i] = j
    y_centres = 0.5 * (y_edges[1:] + y_edges[:-1])
    out.update(ref_line_opacity=op, ref_doi_index=doi_idx, ref_doi_depth=y_centres[doi_idx])
    np.savez_compressed(os.path.join(HERE, "line_products.npz"), **out)
    print("wrote line_products.npz", {k: np.asarray(v).shape for k, v in out.items()})
    print("doi index", doi_idx, "entropy[0][:4]", out["ref_entropy"][0][:4])


if __name__ == "__main__":
    main()
