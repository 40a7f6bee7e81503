"""Sampled unit posteriors, CPU tier: the unit bounds of the interval specs, the host rule (inference.Posteriors(units=..., first=...):
conductance, transverse resistance, depth to a threshold) and the statistics derived from the histograms (unit_posteriors).  The
device accumulators are held against this host rule in tests/test_unit_posteriors_gpu.py."""
import math

import numpy as np
import pytest
import torch

from geobipy_amd import intervals, unit_posteriors
from geobipy_amd.inference import Posteriors, first_layer, unit_kind_bits, unit_means

ULP = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------
# intervals.unit_bounds
# ------------------------------------------------------------------------------------------------------------------
def test_unit_bounds_of_depth_edges():
    z = intervals.unit_bounds(dict(kind="depth", edges=[0.0, 10.0, 30.0, 75.0]), 3, max_depth=165.0)
    assert z.shape == (3, 3, 2) and z.dtype == np.float64
    assert np.array_equal(z[1], [[0.0, 10.0], [10.0, 30.0], [30.0, 75.0]])
    # a unit straddling max_depth is cut there; a unit beyond it has dz == 0
    z = intervals.unit_bounds(dict(kind="depth", edges=[0.0, 100.0, 200.0, 300.0]), 1, max_depth=165.0)
    assert np.array_equal(z[0], [[0.0, 100.0], [100.0, 165.0], [165.0, 165.0]])


def test_unit_bounds_of_elevation_edges_are_ordered_lowest_first():
    surface = np.array([100.0, 35.0, 5.0])
    spec = dict(kind="elevation", edges=[-20.0, 10.0, 40.0, 120.0])
    z = intervals.unit_bounds(spec, 3, surface=surface, max_depth=150.0)
    assert z.shape == (3, 3, 2)
    # sounding 0 (surface 100): units [-20, 10] -> depths [90, 120], [10, 40] -> [60, 90], [40, 120] straddles the surface -> [0, 60]
    assert np.array_equal(z[0], [[90.0, 120.0], [60.0, 90.0], [0.0, 60.0]])
    # sounding 1 (surface 35): [25, 55]; [10, 40] straddles the surface -> [0, 25]; [40, 120] is above the ground -> dz == 0
    assert np.array_equal(z[1], [[25.0, 55.0], [0.0, 25.0], [0.0, 0.0]])
    # sounding 2 (surface 5): [-20, 10] straddles -> [0, 25]; the others are above the ground
    assert np.array_equal(z[2], [[0.0, 25.0], [0.0, 0.0], [0.0, 0.0]])
    # the order is elevation_ranges' (interval 0 the lowest): the deepest unit comes first
    r = intervals.elevation_ranges(surface, np.arange(0.0, 151.0, 1.0), spec["edges"])
    assert np.all(r.lo[0, :-1] >= r.lo[0, 1:]) and np.all(z[0, :-1, 0] >= z[0, 1:, 0])
    # a unit wholly below max_depth
    z = intervals.unit_bounds(spec, 3, surface=surface, max_depth=50.0)
    assert np.array_equal(z[0], [[50.0, 50.0], [50.0, 50.0], [0.0, 50.0]])
    with pytest.raises(ValueError):
        intervals.unit_bounds(spec, 3, max_depth=50.0)           # no surface


def test_unit_bounds_of_horizons():
    top, bottom = np.array([5.0, 20.0, np.nan, 30.0]), np.array([25.0, 400.0, 50.0, 10.0])
    z = intervals.unit_bounds(dict(kind="horizons", top=top, bottom=bottom), 4, max_depth=165.0)
    assert z.shape == (4, 1, 2)
    assert np.array_equal(z[:, 0], [[5.0, 25.0], [20.0, 165.0], [0.0, 0.0], [30.0, 30.0]])     # cut, NaN -> empty, bottom above top -> empty
    # as elevations under a surface: one above the ground, one straddling it
    s = np.array([50.0, 50.0])
    z = intervals.unit_bounds(dict(kind="horizons", top=np.array([80.0, 60.0]), bottom=np.array([55.0, 20.0]), surface=s), 2, max_depth=165.0)
    assert np.array_equal(z[:, 0], [[0.0, 0.0], [0.0, 30.0]])


# ------------------------------------------------------------------------------------------------------------------
# the host rule
# ------------------------------------------------------------------------------------------------------------------
def _random_model(rng, k):
    e = np.cumsum(rng.uniform(0.5, 25.0, size=k - 1)) + 0.3
    return e, 10.0 ** rng.uniform(-3.5, 0.5, size=k)


def _terms(e, s, z0, z1):
    top = np.r_[0.0, e]
    bot = np.r_[e, np.inf]
    ov = np.maximum(0.0, np.minimum(bot, z1) - np.maximum(top, z0))
    keep = ov > 0.0
    return s[keep], ov[keep]


def test_conductance_and_resistance_against_fsum():
    rng = np.random.default_rng(11)
    worst_s = worst_t = 0.0
    n = 0
    for k in range(1, 31):
        for _ in range(20):
            e, s = _random_model(rng, k)
            deepest = e[-1] if k > 1 else 50.0
            for _ in range(6):
                z0 = rng.uniform(0.0, 1.2 * deepest)
                z1 = z0 + rng.uniform(0.01, 1.5 * deepest)
                dz, S, T = unit_means(e, s, z0, z1)
                sl, ov = _terms(e, s, z0, z1)
                fs, ft = math.fsum(float(a * b) for a, b in zip(sl, ov)), math.fsum(float(b / a) for a, b in zip(sl, ov))
                assert dz == np.float64(z1) - np.float64(z0)
                assert abs(S - fs) <= 32 * ULP * fs, (k, S, fs)
                assert abs(T - ft) <= 32 * ULP * ft, (k, T, ft)
                worst_s, worst_t = max(worst_s, abs(S - fs) / fs), max(worst_t, abs(T - ft) / ft)
                assert dz / T <= (S / dz) * (1.0 + 4 * ULP)                  # harmonic <= arithmetic, per sample
                n += 1
    print("unit_means vs fsum over %d cases: worst relative error S %.2e, T %.2e (bound %.2e)" % (n, worst_s, worst_t, 32 * ULP))


def test_unit_inside_one_layer_gives_that_layer():
    rng = np.random.default_rng(3)
    for _ in range(200):
        e, s = _random_model(rng, 6)
        l = int(rng.integers(0, 6))
        top, bot = (0.0 if l == 0 else e[l - 1]), (e[l] if l < 5 else e[-1] + 80.0)
        z0 = top + 0.25 * (bot - top) * rng.uniform()
        z1 = bot - 0.25 * (bot - top) * rng.uniform()
        dz, S, T = unit_means(e, s, z0, z1)
        a, h = S / dz, dz / T
        assert abs(a - s[l]) <= 2 * np.spacing(s[l]) and abs(h - s[l]) <= 2 * np.spacing(s[l])


def test_unit_reaching_into_the_half_space():
    e, s = np.array([10.0, 30.0]), np.array([0.01, 0.1, 1.0])
    dz, S, T = unit_means(e, s, 20.0, 100.0)                     # 10 m of layer 1, 70 m of the half-space (bot = +inf)
    assert dz == 80.0 and S == 0.1 * 10.0 + 1.0 * 70.0 and T == 10.0 / 0.1 + 70.0 / 1.0
    dz, S, T = unit_means(e, s, 50.0, 60.0)                      # wholly inside the half-space
    assert S == 10.0 and T == 10.0
    dz, S, T = unit_means(np.zeros(0), np.array([0.2]), 3.0, 8.0)   # a half-space model
    assert S / dz == 0.2 and dz / T == 0.2
    dz, S, T = unit_means(e, s, 12.0, 12.0)                      # an empty unit
    assert dz == 0.0 and S == 0.0 and T == 0.0


def test_depth_to_a_threshold():
    e, s = np.array([10.0, 30.0]), np.array([0.5, 0.01, 0.2])
    assert first_layer(e, s, 0.1, +1) == 0.0                     # the first layer qualifies: d = 0
    assert first_layer(e, s, 0.1, -1) == 10.0                    # direction -1: the first layer AT OR BELOW the threshold
    assert first_layer(e, s, 0.5, +1) == 0.0 and first_layer(e, s, 0.01, -1) == 10.0      # the bounds are inclusive
    assert first_layer(e, s, 0.6, +1) is None and first_layer(e, s, 0.001, -1) is None
    assert first_layer(e, np.array([0.001, 0.01, 0.2]), 0.1, +1) == 30.0
    p = Posteriors(30, 150.0, 1.0, 0.05, first=([0.1, 0.1, 0.6], [1, -1, 1]))
    p.update(e, s)
    p.update(e, s)
    assert p.first_hist.shape == (3, p.depth_centres.size) and p.first_hist.sum() == 4
    assert p.first_hist[0, 0] == 2 and p.first_hist[1, int(10.0 / 0.5)] == 2          # depth cells of 0.5 minimum_thickness
    assert np.array_equal(p.first_none, [0, 0, 2])                                    # nothing reaches 0.6 S/m: the `none` counter
    p.reset()
    assert p.first_hist.sum() == 0 and p.first_none.sum() == 0


def test_posteriors_accumulate_units_with_the_hit_map_axis():
    units = np.array([[0.0, 10.0], [10.0, 30.0], [12.0, 12.0], [25.0, 400.0]])
    p = Posteriors(30, 150.0, 1.0, 0.05, factor=10.0, n_value_bins=250, units=units, unit_kinds=("arithmetic", "harmonic"))
    assert p.unit_hist.shape == (2, 250, 4)
    e, s = np.array([10.0, 30.0]), np.array([0.5, 0.01, 0.2])
    for _ in range(3):
        p.update(e, s)
    assert np.array_equal(p.unit_hist.sum(axis=1), [[3, 3, 0, 3], [3, 3, 0, 3]])       # the empty unit has no posterior
    # a unit inside one layer lands in the hit map's cell of that layer's conductivity
    col = int(np.searchsorted(p.depth_centres, 5.0))
    assert p.unit_hist[0, :, 0].argmax() == p.values[:, col].argmax() == p.unit_hist[1, :, 0].argmax()
    # harmonic <= arithmetic: the cumulative counts of the harmonic histogram lead
    assert np.all(np.cumsum(p.unit_hist[1], axis=0) >= np.cumsum(p.unit_hist[0], axis=0))
    assert p.unit_hist[1, :, 3].argmax() < p.unit_hist[0, :, 3].argmax()
    one = Posteriors(30, 150.0, 1.0, 0.05, units=units, unit_kinds="harmonic")
    one.update(e, s)
    assert one.unit_hist.shape == (1, 250, 4) and np.array_equal(one.unit_hist[0] * 3, p.unit_hist[1])
    p.reset()
    assert p.unit_hist.sum() == 0
    assert unit_kind_bits(("harmonic", "arithmetic")) == 3 and unit_kind_bits("arithmetic") == 1
    for bad in ([[5.0, 1.0]], [[-1.0, 2.0]], [[0.0, np.inf]], np.zeros((17, 2))):
        with pytest.raises(ValueError):
            Posteriors(30, 150.0, 1.0, 0.05, units=bad)
    for bad in (([0.0], [1]), ([np.nan], [1]), ([0.1], [2]), ([0.1] * 5, [1] * 5)):
        with pytest.raises(ValueError):
            Posteriors(30, 150.0, 1.0, 0.05, first=bad)
    with pytest.raises(ValueError):
        unit_kind_bits(("geometric",))


# ------------------------------------------------------------------------------------------------------------------
# unit_posteriors: what is derived from the histograms' statistics
# ------------------------------------------------------------------------------------------------------------------
def _value_statistics(hist, lmp, hw, percentiles):
    """Host statistics along the value axis of hist [N, n_value, M] (cell centres; a quantile is the first cell at which the
    cumulative count reaches it): only what this file's hand-made, well-separated histograms need."""
    N, nv, M = hist.shape
    centres = (np.arange(nv) + 0.5) / nv * 2.0 * hw - hw
    out = {k: np.full((N, M), np.nan) for k in ("mean", "median", "mode", "credible_range") + tuple("percentile_%g" % p for p in percentiles)}
    out["total"] = hist.sum(axis=1)
    for n in range(N):
        x = centres + lmp[n] / np.log(10.0)
        for m in range(M):
            c = hist[n, :, m]
            if c.sum() == 0:
                continue
            cdf = np.cumsum(c) / c.sum()
            q = lambda f: x[int(np.searchsorted(cdf, f, side="left"))]        # noqa: E731
            out["mean"][n, m], out["mode"][n, m], out["median"][n, m] = (c * x).sum() / c.sum(), x[c.argmax()], q(0.5)
            out["credible_range"][n, m] = q(0.95) - q(0.05)
            for p in percentiles:
                out["percentile_%g" % p][n, m] = q(p * 0.01)
    return {k: torch.as_tensor(v) for k, v in out.items()}


def test_derived_conductance_and_resistance():
    nv, hw, pct = 40, 2.0, (5, 50, 95)
    lmp = np.log(np.array([0.1, 0.02]))
    rng = np.random.default_rng(8)
    dz = np.array([[10.0, 0.0, 45.0], [2.5, 20.0, 100.0]])
    arith = rng.integers(0, 50, size=(2, nv, 3))
    harm = rng.integers(0, 50, size=(2, nv, 3))
    arith[:, :, 1] = 0; harm[0, :, 1] = 0                        # unit 1 of sounding 0: dz == 0; of sounding 1: arithmetic never accumulated
    stats = dict(arithmetic=_value_statistics(arith, lmp, hw, pct), harmonic=_value_statistics(harm, lmp, hw, pct))
    out = unit_posteriors.derive(stats, dz, ("arithmetic", "harmonic"), pct)
    ldz = np.log10(np.where(dz > 0, dz, 1.0))
    live = np.array([[True, False, True], [True, True, True]])
    for k in ("mean", "median", "mode", "percentile_5", "percentile_50", "percentile_95"):
        a, h = stats["arithmetic"][k].numpy(), stats["harmonic"][k].numpy()
        got = out["unit_conductance_" + k].numpy()
        assert np.array_equal(np.isnan(got), ~(live & (arith.sum(axis=1) > 0)))                       # NaN: dz == 0 or nothing accumulated
        ok = ~np.isnan(got)
        assert np.allclose(got[ok], (a + ldz)[ok], rtol=0, atol=1e-14)                               # log10 S = log10 a + log10 dz
        assert np.array_equal(out["unit_arithmetic_" + k].numpy()[ok], a[ok])
        okh = live & (harm.sum(axis=1) > 0)
        assert np.array_equal(out["unit_harmonic_" + k].numpy()[okh], h[okh]) and np.isnan(out["unit_harmonic_" + k].numpy()[~okh]).all()
    h = {k: v.numpy() for k, v in stats["harmonic"].items()}
    okh = live & (harm.sum(axis=1) > 0)
    for p, mirror in ((5, 95), (50, 50), (95, 5)):                 # log10 T = log10 dz - log10 h: the percentiles mirror
        got = out["unit_resistance_percentile_%d" % p].numpy()
        assert np.allclose(got[okh], (ldz - h["percentile_%d" % mirror])[okh], rtol=0, atol=1e-14) and np.isnan(got[~okh]).all()
    assert np.all(out["unit_resistance_percentile_5"].numpy()[okh] <= out["unit_resistance_percentile_95"].numpy()[okh])
    assert np.allclose(out["unit_resistance_mean"].numpy()[okh], (ldz - h["mean"])[okh], rtol=0, atol=1e-14)
    assert np.array_equal(out["unit_resistance_credible_range"].numpy()[okh], h["credible_range"][okh])
    assert np.array_equal(out["unit_thickness"].numpy(), dz)
    assert unit_posteriors.mirrored((5, 50, 95)) == (5.0, 50.0, 95.0) and unit_posteriors.mirrored((10, 50)) == (10.0, 50.0, 90.0)


def test_first_depth_statistics():
    nd, w = 20, 0.5
    fh = np.zeros((2, 2, nd), dtype=np.int32)
    fh[0, 0, 4] = 10                                             # always at cell 4
    fh[0, 1, 2], fh[0, 1, 10] = 30, 70                           # 30 % at cell 2, 70 % at cell 10
    fh[1, 0, 19] = 5                                             # row 1, threshold 1: never a layer
    none = np.array([[0, 100], [15, 40]], dtype=np.int32)
    out = unit_posteriors.first_depth(fh, none, w, (5, 50, 95))
    assert np.array_equal(out["first_depth_median"].numpy()[0], [4.5 * w, 10.5 * w])
    assert np.array_equal(out["first_depth_percentile_5"].numpy()[0], [4.5 * w, 2.5 * w])
    assert np.array_equal(out["first_depth_percentile_95"].numpy()[0], [4.5 * w, 10.5 * w])
    assert out["first_depth_median"].numpy()[1, 0] == 19.5 * w and np.isnan(out["first_depth_median"].numpy()[1, 1])
    assert np.allclose(out["first_probability"].numpy(), [[1.0, 0.5], [0.25, 0.0]])
    empty = unit_posteriors.first_depth(np.zeros((1, 1, nd), dtype=np.int32), np.zeros((1, 1), dtype=np.int32), w)
    assert np.isnan(empty["first_probability"].numpy()).all() and np.isnan(empty["first_depth_median"].numpy()).all()


def test_save_round_trip(tmp_path):
    out = dict(unit_thickness=torch.tensor([[1.0, 2.0]]), first_probability=np.array([[0.5]]))
    path = unit_posteriors.save(out, str(tmp_path / "units.npz"))
    back = np.load(path)
    assert np.array_equal(back["unit_thickness"], [[1.0, 2.0]]) and np.array_equal(back["first_probability"], [[0.5]])


def test_sampler_refuses_bad_unit_arguments_before_touching_the_device():
    """The checks DeviceChains runs on its unit arguments are the host rule's (no GPU needed to refuse them)."""
    from geobipy_amd.inference import check_first, check_unit_bounds
    with pytest.raises(ValueError):
        check_unit_bounds(np.array([[3.0, 1.0]]))
    with pytest.raises(ValueError):
        check_unit_bounds(np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError):
        check_first([0.1, -0.2], [1, 1])
    with pytest.raises(ValueError):
        check_first([0.1], [0])
    t, d = check_first([0.1, 0.3], [1, -1])
    assert t.dtype == np.float64 and np.array_equal(d, [1, -1])
