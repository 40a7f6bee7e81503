#!/usr/bin/env python
"""Reference class (lithology) probabilities of the eight hit maps of line_products.npz (build container only; needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_class_probability.py   ->  tests/golden/class_probability.npz

The posterior is the reference's own ``Histogram`` over a ``RectilinearMesh2D``, built as make_line_products.py builds it (value axis 0:
log10 relative to the prior mean; depth axis 1; its edges and ``relative_to`` are checked against line_products.npz), and each of that
fixture's eight maps is assigned to the counts in turn (the counts are read from it, not duplicated).  For every map and each class
set below, the IMPORTED reference's ``Histogram.compute_probability(MvNormal(mean=means, variance=scales), log=10, axis=0)``
(statistics/Histogram.py:86-87 -> mesh/RectilinearMesh2D.py:313-344) is recorded, [K, n_depth] per map, with numpy's argmax / the
probability at it over the class axis (Inference2D.highestMarginal / probability_of_highest_marginal).

The reference's ``MvNormal.probability`` builds ``Normal(...)`` without a prng, and ``baseDistribution`` asserts on that; the recorder gives
``baseDistribution.__init__`` a default ``np.random.Generator(np.random.PCG64DXSM(0))`` to let the call run.  The probabilities draw no
random numbers, so the patch cannot change them.  The reference hands the "variance" to scipy's ``norm.pdf`` as the SCALE
(MvNormalDistribution.py:183-199 -> NormalDistribution.py:125-134): the scales here are standard deviations.  No set has K equal to the
number of value cells (where ``MvNormal.probability`` takes its multivariate branch).

Class sets, in log10 S/m around the maps' value range [lo, hi]:
  a  K = 1;
  b  K = 3, moderate scales over the range;
  c  K = 8, classes 2 and 5 identical (argmax ties: the first wins);
  d  K = 16, narrow scales (0.02);
  e  K = 2, far outside the range: every term underflows to 0, every column NaN.
The recorder asserts that in every column either all terms c_v phi_k(x_v) are exactly 0 or the largest is a normal float, so that no
subnormal rounding enters the comparison.  The fixture holds data only.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference   # noqa: E402


def class_sets(lo, hi):
    import numpy as np
    span = hi - lo
    c8 = list(np.linspace(lo + 0.1 * span, hi - 0.1 * span, 8))
    c8[5] = c8[2]
    s8 = [0.15 * span] * 8
    s8[2] = s8[5] = 0.1 * span
    return dict(
        a=([lo + 0.3 * span], [0.2 * span]),
        b=([lo + 0.25 * span, lo + 0.5 * span, lo + 0.8 * span], [0.1 * span, 0.08 * span, 0.12 * span]),
        c=(c8, s8),
        d=(list(lo + (np.arange(16) + 0.5) / 16 * span), [0.02] * 16),
        e=([hi + 60.0, lo - 70.0], [0.5, 0.3]),
    )


def posterior():
    """The reference's conductivity-depth posterior Histogram, built as make_line_products.py builds it (the mesh of its fixture)."""
    from make_golden import REF, SUP
    from geobipy import FdemData, Inference1D, get_prng
    from geobipy.src.inversion import user_parameters as up
    opt_file = REF + "/documentation_source/source/supplementary/options_files/resolve_options"
    options = up.user_parameters.read(opt_file, data_directory=SUP)
    options["system_filename"] = SUP + "/resolve.stm"
    options["n_markov_chains"] = 100
    options["save_hdf5"] = False
    options["interactive_plot"] = True
    options["update_plot_every"] = 100000
    data = FdemData.read_csv(SUP + "/resolve_glacial.csv", system=options["system_filename"])
    inf = Inference1D(prng=get_prng(seed=options["seed"] if "seed" in options else 1), **options)
    inf.initialize(data.datapoint(30))
    return inf.model.values.posterior


def main():
    import numpy as np
    from scipy.stats import norm
    import_reference()
    from geobipy.src.classes.statistics import baseDistribution as bd
    from geobipy.src.classes.statistics.MvNormalDistribution import MvNormal

    def _init(self, prng=None):
        self.prng = np.random.Generator(np.random.PCG64DXSM(0)) if prng is None else prng
    bd.baseDistribution.__init__ = _init

    lp = dict(np.load(os.path.join(HERE, "line_products.npz")))
    counts = lp["counts"]                                         # [8, n_value, n_depth]
    nv, nz = counts.shape[1:]
    h = posterior()
    mesh = h.mesh
    assert np.array_equal(np.asarray(mesh.x.edges, dtype=np.float64), lp["x_edges"])
    assert np.array_equal(np.asarray(mesh.y.edges, dtype=np.float64), lp["y_edges"])
    rel = float(np.asarray(mesh.x.relative_to).ravel()[0])
    assert rel == float(lp["relative_to"])
    xc = np.log10(np.asarray(mesh.centres(axis=0), dtype=np.float64))
    lo, hi = float(xc.min()), float(xc.max())
    print("value cells", nv, "depth cells", nz, "relative_to", rel, "log10 centres", lo, "..", hi)

    out = dict(sets=np.array(sorted(class_sets(lo, hi))))
    for name, (means, scales) in sorted(class_sets(lo, hi).items()):
        mu, sd = np.asarray(means, dtype=np.float64), np.asarray(scales, dtype=np.float64)
        assert mu.size != nv
        phi = np.stack([norm.pdf(xc, loc=m, scale=s) for m, s in zip(mu, sd)])          # [K, n_value]
        prob, best, best_p = [], [], []
        for c in counts:
            terms = c[None, :, :] * phi[:, :, None]                                      # [K, n_value, n_depth]
            big = terms.reshape(-1, nz).max(axis=0)
            assert np.all((big == 0.0) | (big >= np.finfo(np.float64).tiny)), name
            h.values = c.astype(np.int32)
            p = np.asarray(h.compute_probability(MvNormal(mean=mu, variance=sd), log=10, axis=0, track=False), dtype=np.float64)
            assert p.shape == (mu.size, nz), p.shape
            j = np.argmax(p, axis=0)
            prob.append(p)
            best.append(j.astype(np.int32))
            best_p.append(np.take_along_axis(p, j[None], axis=0)[0])
        out.update({"means_" + name: mu, "scales_" + name: sd, "prob_" + name: np.stack(prob), "best_" + name: np.stack(best),
                    "best_p_" + name: np.stack(best_p)})
        print(name, "K", mu.size, "NaN columns", int(np.isnan(out["best_p_" + name]).sum()), "of", len(counts) * nz)
    np.savez_compressed(os.path.join(HERE, "class_probability.npz"), **out)
    print("wrote class_probability.npz", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
