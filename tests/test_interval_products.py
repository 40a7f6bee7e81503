"""Interval (unit) posteriors: the marginal hit maps over depth and elevation ranges and their statistics (csrc/gbp_hitmap.h
k_hitmap_intervals and the int64 instances of k_hitmap_products / k_hitmap_classes, geobipy_amd/intervals.py,
hitmap.interval_marginals, line_products.from_results(intervals=...), survey_volume.from_lines(intervals=...)).

CPU tier: (i) the numpy / torch statement (tests/interval_reference.py) and the range builders against the imported REFERENCE's own
numbers (tests/golden/make_interval_products.py -> interval_products.npz): cell ranges, ``n_cells``, marginals, the mode's cell and the
classes' argmax exactly; percentiles to 1e-9 of a value cell, the credible range to 1e-12, probabilities to rtol 1e-10 (floor 1e-250)
-- the tolerances of test_line_products.py and test_class_probability.py for the same quantities.  The mean is held to 1e-12, the
tolerance test_hitmap_gpu.py holds the per-cell mean to the reference at: the reference returns 10 ** mean, so the recorded log10 of
it cannot carry the bits of a sum / total (measured here: max |difference| 1.3e-15 over the three cases).  The mode is compared both
as a float (1e-9 of a cell) and as the cell index recovered from the reference's float, which is exact.  (ii) The range builders
against brute-force membership on random axes with coincident boundaries; (iii) the command lines' arguments; (iv) the C ABI's
refusals.

GPU tier: the kernel and the 64-bit entries against the fixture and against the statement on many shapes; the identity (edges = the
depth edges: the marginals are the maps, every interval product has the bits of the per-cell product); int64 and int32 instances give
the same bits; ``from_results`` / ``from_lines`` / both command lines end to end on the committed line container; ``interval_*``
entries pass ``on_elevation`` unchanged."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import interval_reference as ir

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "interval_products.npz")
MAPS = os.path.join(HERE, "golden", "line_products.npz")
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")
CASES = ("partition", "elevation", "pairs")
RTOL, ATOL = 1e-10, 1e-250                       # test_class_probability.py
CLASSES = ([-2.5, -1.5, -0.5], [0.3, 0.3, 0.4])


def _fixture():
    import torch
    d = dict(np.load(GOLDEN))
    m = dict(np.load(MAPS))
    W = float(m["x_edges"][-1])
    counts = torch.as_tensor(m["counts"])
    lmp = torch.full((counts.shape[0],), float(m["relative_to"]) * np.log(10.0), dtype=torch.float64)
    return d, m, counts, lmp, W


def _ranges(d, m, case):
    """The package's ranges [8, M] for the fixture's case."""
    from geobipy_amd import intervals as iv
    n = m["counts"].shape[0]
    if case == "partition":
        r = iv.depth_ranges(m["y_edges"], d["partition_edges"])
    elif case == "pairs":
        r = iv.depth_pairs(m["y_edges"], d["pairs"])
    else:
        return iv.elevation_ranges(d["surfaces"], m["y_edges"], d["elevation_edges"])
    return iv.Ranges(*(np.broadcast_to(a, (n, a.size)) for a in r))


def _same_probabilities(got, want, tag=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str(tag))


def _hold_products_to_fixture(out, d, m, case, W, n_cells):
    """``out``: {name: numpy [8, M]} with mean, mode, percentile_<p>, credible_range (NaN where no cells)."""
    nv = m["counts"].shape[1]
    cell = 2.0 * W / nv
    has = n_cells > 0
    free = has & ~d["ties_" + case]
    for k in ("mean", "mode", "credible_range"):
        assert np.isnan(out[k][~has]).all() and not np.isnan(out[k][has]).any(), (case, k)
    err = np.abs(out["mean"] - d["ref_mean_" + case])[has].max()
    print(case, "max |mean - reference|", err)
    assert err < 1e-12, (case, err)
    assert np.abs(out["mode"] - d["ref_mode_" + case])[has].max() < 1e-9 * cell, case
    ref_idx = np.rint((d["ref_mode_" + case] - float(m["relative_to"]) + W) / cell - 0.5).astype(np.int64)
    idx = out["mode_idx"] if "mode_idx" in out else np.rint((np.where(has, out["mode"], 0.0) - float(m["relative_to"]) + W) / cell - 0.5).astype(np.int64)
    assert np.array_equal(idx[has], ref_idx[has]), case
    for k, p in enumerate(d["percentiles"]):
        assert np.abs(out["percentile_%g" % p] - d["ref_percentiles_" + case][:, k])[free].max() < 1e-9 * cell, (case, p)
    assert np.abs(out["credible_range"] - d["ref_credible_range_" + case])[free].max() < 1e-12, case


def _hold_classes_to_fixture(out, d, case, name, n_cells):
    has = (n_cells > 0)
    P = np.asarray(out["probability"])
    want = d["prob_%s_%s" % (name, case)]
    mask = np.broadcast_to(has[:, None, :], P.shape)
    _same_probabilities(np.where(mask, P, 0.0), np.where(mask, want, 0.0), (case, name))
    assert np.array_equal(np.asarray(out["highest_marginal"])[has], d["best_%s_%s" % (name, case)][has]), (case, name)
    _same_probabilities(np.asarray(out["probability_of_highest_marginal"])[has], d["best_p_%s_%s" % (name, case)][has], (case, name))


def test_fixture_holds_the_cases_the_issue_names():
    d, m, counts, lmp, W = _fixture()
    e = m["y_edges"]
    c = 0.5 * (e[1:] + e[:-1])
    pe = d["partition_edges"]
    assert any(v in c for v in pe[:-1]) and any(v in e for v in pe) and pe[-1] in c          # on a centre, on an edge, the closed last edge
    n_cells = d["hi_partition"] - d["lo_partition"]
    assert (n_cells[:, 0] == 0).all() and pe[1] < e[0]                                         # above the surface
    assert (n_cells == 1).any()
    assert d["marginals_partition"].dtype == np.int64 and d["marginals_partition"][6].sum(axis=0).max() > 2 ** 31
    ne = d["hi_elevation"] - d["lo_elevation"]
    assert (ne[:, -1] == 0).any() and (ne[:, 0] == 0).any()                                    # above the surface, below the mesh
    assert any(np.any(s - c == v) for s in d["surfaces"] for v in d["elevation_edges"])       # an elevation edge on a cell centre
    assert np.unique(d["surfaces"]).size == d["surfaces"].size
    lo, hi = d["lo_pairs"][0], d["hi_pairs"][0]
    assert np.any((lo[:, None] < hi[None, :]) & (lo[None, :] < hi[:, None]) & ~np.eye(lo.size, dtype=bool))      # overlapping pairs
    marked = sum(int(d["ties_" + k].sum()) for k in CASES)
    full = sum(int((d["marginals_" + k].sum(axis=1) > 0).sum()) for k in CASES)
    empty = sum(int((d["hi_" + k] - d["lo_" + k] == 0).sum()) for k in CASES)
    total = sum(d["lo_" + k].size for k in CASES)
    assert 0 < marked <= 0.10 * full and empty <= 0.25 * total, (marked, full, empty, total)
    assert list(d["census"]) == [marked, full, empty, total]


@pytest.mark.parametrize("case", CASES)
def test_ranges_and_statement_equal_the_reference(case):
    import torch
    d, m, counts, lmp, W = _fixture()
    r = _ranges(d, m, case)
    n_cells = d["hi_" + case] - d["lo_" + case]
    assert np.array_equal(r.n_cells, n_cells) and r.n_cells.dtype == np.int32
    has = n_cells > 0
    assert np.array_equal(r.lo[has], d["lo_" + case][has]) and np.array_equal(r.hi[has], d["hi_" + case][has])
    marg = ir.marginals_numpy(m["counts"], r.lo, r.hi)
    assert np.array_equal(marg, d["marginals_" + case])
    mt = ir.marginals_torch(counts, torch.as_tensor(r.lo.copy()), torch.as_tensor(r.hi.copy()))
    assert mt.dtype == torch.int64 and np.array_equal(mt.numpy(), marg)
    out = ir.products_torch(mt, lmp, W, tuple(d["percentiles"]), float(d["credible"]), n_cells=n_cells)
    _hold_products_to_fixture(out, d, m, case, W, n_cells)
    for name in d["sets"]:
        c = ir.classes_torch(mt, lmp, W, d["means_" + name], d["scales_" + name])
        _hold_classes_to_fixture({k: v.numpy() for k, v in c.items()}, d, case, name, n_cells)


def _random_depth_edges(rng, nz):
    steps = rng.choice([0.25, 0.5, 1.0, 2.0], nz)
    return np.concatenate([[0.0], np.cumsum(steps)])


def test_range_builders_equal_brute_force_membership():
    from geobipy_amd import intervals as iv
    rng = np.random.default_rng(31)
    for trial in range(60):
        nz = int(rng.integers(1, 40))
        e = _random_depth_edges(rng, nz)
        c = 0.5 * (e[1:] + e[:-1])
        assert iv.depth_centres(e).tobytes() == c.tobytes()
        M = int(rng.integers(1, 9))
        # edges drawn from the cell centres, the cell edges and free values: boundaries coincide with both
        pool = np.concatenate([c, e, rng.uniform(-5.0, e[-1] + 5.0, 6)])
        x = np.unique(rng.choice(pool, M + 1, replace=False))
        if x.size < 2:
            continue
        r = iv.depth_ranges(e, x)
        for k in range(x.size - 1):
            lo, hi = ir.as_range(ir.members(c, x[k], x[k + 1], closed=k == x.size - 2))
            assert r.n_cells[k] == hi - lo and (hi == lo or (r.lo[k], r.hi[k]) == (lo, hi)), (trial, k)
        # elevation: per-sounding surfaces, some chosen to put a centre exactly on an edge
        N = 5
        xe = np.unique(np.round(rng.uniform(-e[-1] - 3.0, 6.0, M + 1) * 4.0) / 4.0)
        if xe.size >= 2:
            s = np.concatenate([rng.uniform(-2.0, 4.0, N - 2), [xe[-1] + c[0], xe[0] + c[-1]]])
            re_ = iv.elevation_ranges(s, e, xe)
            assert re_.lo.shape == (N, xe.size - 1)
            for n in range(N):
                el = s[n] - c
                for k in range(xe.size - 1):
                    lo, hi = ir.as_range(ir.members(el, xe[k], xe[k + 1], closed=k == xe.size - 2))
                    assert re_.n_cells[n, k] == hi - lo and (hi == lo or (re_.lo[n, k], re_.hi[n, k]) == (lo, hi)), (trial, n, k)
            assert (re_.n_cells[N - 2, -1] >= 1) and (re_.n_cells[N - 1, 0] >= 1)        # the closed last edge; a centre on the first edge
        # horizons: depths, and elevations under a surface; NaN and inverted bounds give nothing
        top = rng.choice(pool, (N, 3))
        bot = rng.choice(pool, (N, 3))
        top[0, 0], bot[1, 1] = np.nan, np.nan
        rh = iv.horizon_ranges(e, top, bot)
        s = rng.uniform(-2.0, 4.0, N)
        rs = iv.horizon_ranges(e, s[:, None] - top, s[:, None] - bot, surface=s)
        for n in range(N):
            for k in range(3):
                ok = not (np.isnan(top[n, k]) or np.isnan(bot[n, k]))
                lo, hi = ir.as_range((c >= top[n, k]) & (c < bot[n, k])) if ok else (0, 0)
                assert rh.n_cells[n, k] == hi - lo and (hi == lo or (rh.lo[n, k], rh.hi[n, k]) == (lo, hi)), (trial, n, k)
                el, t_el, b_el = s[n] - c, s[n] - top[n, k], s[n] - bot[n, k]
                lo, hi = ir.as_range((el <= t_el) & (el > b_el)) if ok else (0, 0)
                assert rs.n_cells[n, k] == hi - lo and (hi == lo or (rs.lo[n, k], rs.hi[n, k]) == (lo, hi)), (trial, n, k)
        one = iv.horizon_ranges(e, top[:, 0], bot[:, 0])
        assert one.lo.shape == (N, 1) and np.array_equal(one.n_cells[:, 0], rh.n_cells[:, 0])
        # pairs: the cells holding both depths and those between (survey_volume.depth_cells); beyond the mesh: what is inside
        a, b = np.sort(rng.uniform(e[0], e[-1] * 0.999, 2))
        rp = iv.depth_pairs(e, [[a, b], [b, a], [-3.0, a], [b, e[-1] + 4.0], [e[-1], e[-1] + 1.0], [-2.0, -1.0]])
        ca, cb = np.searchsorted(e, a, side="right") - 1, np.searchsorted(e, b, side="right") - 1
        assert (rp.lo[0], rp.hi[0]) == (ca, cb + 1) == (rp.lo[1], rp.hi[1])
        assert (rp.lo[2], rp.hi[2]) == (0, ca + 1) and (rp.lo[3], rp.hi[3]) == (cb, nz)
        assert rp.n_cells[4] == 0 and rp.n_cells[5] == 0
        ri = iv.depth_pairs(e, np.array([[0, nz - 1], [nz - 1, 0], [0, nz + 5]]))
        assert np.array_equal(ri.lo, [0, 0, 0]) and np.array_equal(ri.hi, [nz, nz, nz])
    for bad in ([1.0], [2.0, 1.0], [0.0, np.nan], [0.0, 0.0]):
        with pytest.raises(ValueError):
            iv.depth_ranges([0.0, 1.0, 2.0], bad)
    with pytest.raises(ValueError):
        iv.depth_ranges([0.0, 2.0, 1.0], [0.0, 1.0])


def test_specs():
    from geobipy_amd import intervals as iv
    s = iv.check_spec({"kind": "depth", "edges": [0, 10, 30]})
    assert s["kind"] == "depth" and s["edges"].dtype == np.float64 and iv.n_intervals(s) == 2
    r = iv.ranges(s, np.arange(0.0, 41.0), 3)
    assert r.lo.shape == (3, 2) and r.lo.tolist() == [[0, 10]] * 3 and r.hi.tolist() == [[10, 30]] * 3
    desc = iv.describe(s)
    assert str(desc["interval_kind"]) == "depth" and np.array_equal(desc["interval_edges"], [0, 10, 30])
    assert iv.same_spec(desc, s) and not iv.same_spec(desc, iv.check_spec({"kind": "depth", "edges": [0, 10, 31]}))
    assert not iv.same_spec(desc, iv.check_spec({"kind": "elevation", "edges": [0, 10, 30]})) and not iv.same_spec({}, s)
    assert iv.n_intervals(iv.check_spec({"kind": "pairs", "pairs": [[0.0, 5.0], [2.0, 9.0], [1.0, 3.0]]})) == 3
    e = iv.check_spec({"kind": "elevation", "edges": [-10.0, 0.0]})
    with pytest.raises(ValueError, match="surface"):
        iv.ranges(e, np.arange(0.0, 41.0), 3)
    assert iv.ranges(e, np.arange(0.0, 41.0), 2, surface=[5.0, 50.0]).n_cells.tolist() == [[10], [0]]
    hz = iv.check_spec({"kind": "horizons", "top": [1.0, 2.0], "bottom": [4.0, np.nan]})
    assert iv.ranges(hz, np.arange(0.0, 41.0), 2).n_cells.tolist() == [[3], [0]]
    for bad in ({"kind": "depths", "edges": [0, 1]}, {"kind": "depth"}, {"kind": "depth", "edges": [1, 0]}, {"kind": "depth", "pairs": [[0, 1]]},
                {"kind": "pairs", "pairs": [0, 1]}, {"kind": "horizons", "top": [1.0]}, {"edges": [0, 1]}):
        with pytest.raises(ValueError):
            iv.check_spec(bad)


def test_command_line_arguments():
    from geobipy_amd import line_products as lp, survey_volume as sv
    a = lp.parse_args(["x.h5"])
    assert a.intervals is None and a.depth_intervals is None and a.elevation_intervals is None
    a = lp.parse_args(["x.h5", "--depth-intervals", "0", "10", "30", "75"])
    assert a.intervals["kind"] == "depth" and a.intervals["edges"].tolist() == [0.0, 10.0, 30.0, 75.0]
    a = lp.parse_args(["x.h5", "--elevation-intervals", "-40", "-10", "--class-means", "-1", "--class-scales", "0.5"])
    assert a.intervals["kind"] == "elevation" and a.intervals["edges"].tolist() == [-40.0, -10.0] and a.class_means == [-1.0]
    v = sv.parse_args(["d", "--dx", "5", "--dy", "5"])
    assert v.intervals is None
    v = sv.parse_args(["d", "--dx", "5", "--dy", "5", "--elevation-intervals", "-40", "-10", "20", "--variables", "mean", "median"])
    assert v.intervals["kind"] == "elevation" and v.intervals["edges"].tolist() == [-40.0, -10.0, 20.0]
    v = sv.parse_args(["d", "--dx", "5", "--dy", "5", "--depth-intervals", "0", "10"])
    assert v.intervals["kind"] == "depth"
    for tail in (["--depth-intervals", "5"], ["--depth-intervals", "10", "5"], ["--depth-intervals", "0", "0"], ["--depth-intervals", "0", "nan"],
                 ["--elevation-intervals", "0", "inf"], ["--elevation-intervals", "3"], ["--depth-intervals"],
                 ["--depth-intervals", "0", "10", "--elevation-intervals", "-10", "0"]):
        with pytest.raises(SystemExit):
            lp.parse_args(["x.h5"] + tail)
        with pytest.raises(SystemExit):
            sv.parse_args(["d", "--dx", "5", "--dy", "5"] + tail)
    with pytest.raises(SystemExit):
        lp.parse_args(["x.h5", "--depth-intervals", "0", "10", "--elevation-axis", "2"])
    for sel in (["--depth", "7"], ["--depth-cells", "1", "4"], ["--elevation-axis", "2"], ["--elevation", "30"]):
        for flag in ("--depth-intervals", "--elevation-intervals"):
            with pytest.raises(SystemExit):
                sv.parse_args(["d", "--dx", "5", "--dy", "5", flag, "0", "10"] + sel)
    assert sv.intervals_volume_path("/o", "mean") == "/o/survey_volume.intervals.mean.npy"


def test_python_entries_refuse_host_tensors_and_bad_input():
    import torch
    from geobipy_amd import _lib, hitmap, survey_volume as sv
    hm = torch.zeros((1, 4, 3), dtype=torch.int32)
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.interval_marginals(hm, torch.tensor([0]), torch.tensor([2]))
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.products(hm.to(torch.int64), torch.zeros(1, dtype=torch.float64), 1.0)
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.class_probability(hm.to(torch.int64), torch.zeros(1, dtype=torch.float64), 1.0, [0.0], [1.0])
    for kw in (dict(depth=3), dict(elevation=10.0), dict(elevation_edges=[0.0, 1.0])):
        with pytest.raises(ValueError, match="excludes"):
            sv.from_lines(SURVEY, 5.0, 5.0, intervals={"kind": "depth", "edges": [0, 10]}, **kw)
    with pytest.raises(ValueError):
        sv.from_lines(SURVEY, 5.0, 5.0, intervals={"kind": "horizons", "top": [1.0] * 8, "bottom": [2.0] * 8})
    with pytest.raises(ValueError, match="units"):
        sv._columns([("x", {"interval_mean": np.zeros((2, 440))})], "interval_mean", 440)


def _lib_or_skip():
    from geobipy_amd import _lib
    try:
        return _lib, _lib.load()
    except (_lib.NativeLibraryError, OSError) as e:
        pytest.skip("native library not loadable here: %s" % e)


def test_c_abi_refuses_bad_arguments():
    _lib, lib = _lib_or_skip()
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, nv=250, nz=440, M=8, hm=p, lo=p, hi=p, out=p):
        return lib.gbp_hitmap_intervals(B, nv, nz, M, hm, lo, hi, out, None)

    assert call(B=0, hm=None, lo=None, hi=None, out=None) == 0                   # an empty block: no launch
    assert call(B=0, M=1024, hm=None, lo=None, hi=None, out=None) == 0 and call(B=0, M=1, hm=None, lo=None, hi=None, out=None) == 0
    assert call(B=-1) == INVALID
    assert call(nv=0) == INVALID and call(nz=0) == INVALID and call(nz=-2) == INVALID
    assert call(M=0) == INVALID and call(M=-1) == INVALID and call(M=4097) == INVALID
    assert call(B=0, M=0, hm=None, lo=None, hi=None, out=None) == INVALID        # (checked before B == 0)
    assert call(nz=1025) == INVALID
    assert call(hm=None) == INVALID and call(lo=None) == INVALID and call(hi=None) == INVALID and call(out=None) == INVALID
    assert b"gbp_hitmap_intervals" in lib.gbp_last_error()
    # the 64-bit entries refuse what the 32-bit ones refuse
    d = (ctypes.c_double * 8)(0.05, 0.5, 0.95)
    assert lib.gbp_hitmap_products_i64(1, 250, 8, None, p, 1.0, 3, d, p, p, p, p, p, None) == INVALID
    assert lib.gbp_hitmap_products_i64(1, 250, 8, p, p, 1.0, 9, d, p, p, p, p, p, None) == INVALID
    assert lib.gbp_hitmap_products_i64(0, 250, 8, None, None, 1.0, 3, d, None, None, None, None, None, None) == 0
    mu, sd = (ctypes.c_double * 2)(-1.0, 0.0), (ctypes.c_double * 2)(0.3, 0.0)
    assert lib.gbp_hitmap_classes_i64(1, 250, 8, p, p, 1.0, 2, mu, sd, p, p, p, None) == INVALID      # a zero scale
    assert lib.gbp_hitmap_classes_i64(1, 250, 8, None, p, 1.0, 1, mu, sd, p, p, p, None) == INVALID
    assert lib.gbp_hitmap_classes_i64(0, 250, 8, None, None, 1.0, 1, mu, sd, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_kernels_equal_the_reference(case):
    import torch
    from geobipy_amd import hitmap
    d, m, counts, lmp, W = _fixture()
    dev = torch.device("cuda", 0)
    r = _ranges(d, m, case)
    n_cells = d["hi_" + case] - d["lo_" + case]
    marg = hitmap.interval_marginals(counts.to(dev), torch.as_tensor(r.lo.copy()), torch.as_tensor(r.hi.copy()))
    assert marg.dtype == torch.int64 and marg.is_cuda and np.array_equal(marg.cpu().numpy(), d["marginals_" + case])
    p = hitmap.products(marg, lmp.to(dev), W, percentiles=tuple(d["percentiles"]), credible=float(d["credible"]))
    out = {k: np.where(n_cells == 0, np.nan, v.cpu().numpy()) for k, v in p.items() if v.dtype.is_floating_point}
    _hold_products_to_fixture(out, d, m, case, W, n_cells)
    assert np.array_equal(p["total"].cpu().numpy(), d["marginals_" + case].sum(axis=1))
    for name in d["sets"]:
        c = hitmap.class_probability(marg, lmp.to(dev), W, d["means_" + name], d["scales_" + name])
        _hold_classes_to_fixture({k: v.cpu().numpy() for k, v in c.items()}, d, case, name, n_cells)


def _maps(rng, B, nv, nz):
    hm = np.zeros((B, nv, nz), dtype=np.int32)
    for b in range(B):
        kind = b % 5
        if kind == 0:                                                          # layered posteriors
            for _ in range(20):
                v, (lo, hi) = rng.integers(0, nv), np.sort(rng.integers(0, nz, 2))
                hm[b, v, lo:hi + 1] += rng.integers(1, 900)
        elif kind == 1:                                                        # dense random
            hm[b] = rng.integers(0, 50, (nv, nz))
        elif kind == 2:                                                        # the largest counts an int32 holds: sums far beyond 2^31
            hm[b] = rng.integers((1 << 31) - 1000, (1 << 31) - 1, (nv, nz), endpoint=True)
        elif kind == 3:                                                        # counts of a long chain
            hm[b] = rng.integers(1 << 22, 1 << 23, (nv, nz)) * (rng.random((nv, nz)) < 0.5)
        # kind 4: empty
    return hm


def _random_ranges(rng, B, M, nz, shared):
    """Overlapping, empty (hi <= lo) and out-of-bounds ranges (the kernel clamps)."""
    shape = (M,) if shared else (B, M)
    lo = rng.integers(-5, nz + 5, shape)
    hi = lo + rng.integers(-3, nz + 8, shape)
    whole = rng.random(shape) < 0.1
    lo, hi = np.where(whole, -7, lo), np.where(whole, nz + 9, hi)
    return lo.astype(np.int64), hi.astype(np.int64)


SHAPES = [(1, 250, 440), (1, 3, 1), (3, 7, 63), (5, 9, 255), (5, 4, 257), (2, 6, 441), (4, 5, 512), (2, 3, 513), (2, 3, 1000), (2, 2, 1024),
          (3, 33, 256), (3000, 5, 440), (2500, 2, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,nv,nz", SHAPES)
def test_interval_kernel_equals_the_statement(B, nv, nz):
    import torch
    from geobipy_amd import hitmap
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(B * 1000003 + nv * 1009 + nz)
    hm = torch.as_tensor(_maps(rng, B, nv, nz), device=dev)
    Ms = (1, 7, 64, nz, 1024) if B < 100 else (1, 7, 64)
    for M in Ms:
        for shared in (True, False):
            lo, hi = _random_ranges(rng, B, M, nz, shared)
            got = hitmap.interval_marginals(hm, torch.as_tensor(lo), torch.as_tensor(hi))
            want = ir.marginals_torch(hm, torch.as_tensor(lo), torch.as_tensor(hi))
            assert got.shape == (B, nv, M) and got.dtype == torch.int64
            assert torch.equal(got, want), (B, nv, nz, M, shared)
    # a view that is not 16-byte aligned takes the unaligned instance
    if nz % 4 == 0 and B > 1:
        flat = torch.zeros(hm.numel() + 1, dtype=torch.int32, device=dev)
        off = flat[1:].view(hm.shape)
        off.copy_(hm)
        assert off.data_ptr() % 16 != 0
        lo, hi = _random_ranges(rng, B, 7, nz, False)
        assert torch.equal(hitmap.interval_marginals(off, torch.as_tensor(lo), torch.as_tensor(hi)),
                           ir.marginals_torch(hm, torch.as_tensor(lo), torch.as_tensor(hi)))


@pytest.mark.gpu
def test_interval_kernel_limits():
    import torch
    from geobipy_amd import _lib, hitmap
    dev = torch.device("cuda", 0)
    hm = torch.ones((2, 3, 8), dtype=torch.int32, device=dev)
    assert hitmap.interval_marginals(hm, torch.zeros(4096, dtype=torch.int64), torch.full((4096,), 8)).eq(8).all()
    with pytest.raises(_lib.NativeLibraryError, match="M outside"):
        hitmap.interval_marginals(hm, torch.zeros(4097, dtype=torch.int64), torch.full((4097,), 8))
    with pytest.raises(_lib.NativeLibraryError, match="M outside"):
        hitmap.interval_marginals(hm, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(_lib.NativeLibraryError, match="n_depth"):
        hitmap.interval_marginals(torch.ones((1, 2, 1025), dtype=torch.int32, device=dev), torch.tensor([0]), torch.tensor([5]))
    with pytest.raises(ValueError):
        hitmap.interval_marginals(hm, torch.zeros((3, 4), dtype=torch.int64), torch.ones((3, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        hitmap.interval_marginals(hm, torch.tensor([0.0]), torch.tensor([2.0]))
    with pytest.raises(TypeError):
        hitmap.interval_marginals(hm.to(torch.int64), torch.tensor([0]), torch.tensor([2]))
    empty = hitmap.interval_marginals(torch.zeros((0, 3, 8), dtype=torch.int32, device=dev), torch.tensor([0, 1]), torch.tensor([2, 3]))
    assert empty.shape == (0, 3, 2)


@pytest.mark.gpu
def test_identity_the_depth_edges_as_intervals():
    import torch
    from geobipy_amd import hitmap, intervals as iv
    d, m, counts, lmp, W = _fixture()
    dev = torch.device("cuda", 0)
    hm, lmp = counts.to(dev), lmp.to(dev)
    r = iv.depth_ranges(m["y_edges"], m["y_edges"])
    nz = hm.shape[2]
    assert np.array_equal(r.lo, np.arange(nz)) and np.array_equal(r.hi, np.arange(nz) + 1)
    marg = hitmap.interval_marginals(hm, torch.as_tensor(r.lo), torch.as_tensor(r.hi))
    assert torch.equal(marg, hm.to(torch.int64))
    pct, cred = tuple(m["percentiles"]), float(m["credible"])
    a, b = hitmap.products(hm, lmp, W, percentiles=pct, credible=cred), hitmap.products(marg, lmp, W, percentiles=pct, credible=cred)
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    for name in d["sets"]:
        ca = hitmap.class_probability(hm, lmp, W, d["means_" + name], d["scales_" + name])
        cb = hitmap.class_probability(marg, lmp, W, d["means_" + name], d["scales_" + name])
        for k in ca:
            assert ca[k].cpu().numpy().tobytes() == cb[k].cpu().numpy().tobytes(), (name, k)


@pytest.mark.gpu
def test_int64_and_int32_instances_give_the_same_bits():
    import torch
    from geobipy_amd import hitmap
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    qsets = ([0.05, 0.5, 0.9500000000000001], [0.01, 0.16, 0.25, 0.5, 0.75, 0.84, 0.99, 0.999], [])
    n = 0
    for B, nv, nz in ((1, 1, 1), (3, 250, 440), (7, 257, 255), (37, 16, 257), (5, 1000, 64)):
        hm = torch.as_tensor(_maps(rng, B, nv, nz), device=dev)
        lmp = torch.as_tensor(rng.normal(-4.0, 0.5, B), device=dev)
        a, b = hitmap.moments(hm, lmp, 2.3, qsets[n % 3]), hitmap.moments(hm.to(torch.int64), lmp, 2.3, qsets[n % 3])
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), (B, nv, nz, k)
        K = (1, 2, 5, 8, 16)[n % 5]
        while K * nv > 8192:                                                   # (the class table's 64 KiB of LDS)
            K //= 2
        means, scales = rng.uniform(-7.0, -1.0, K), rng.uniform(0.05, 1.0, K)
        ca, cb = hitmap.class_probability(hm, lmp, 2.3, means, scales), hitmap.class_probability(hm.to(torch.int64), lmp, 2.3, means, scales)
        for k in ca:
            assert ca[k].cpu().numpy().tobytes() == cb[k].cpu().numpy().tobytes(), (B, nv, nz, K, k)
        n += 1
    # and beyond int32: marginals of the largest counts against the statement
    hm = torch.as_tensor(_maps(rng, 5, 40, 440), device=dev)
    lo, hi = torch.tensor([0, 100, 3]), torch.tensor([440, 300, 4])
    marg = hitmap.interval_marginals(hm, lo, hi)
    assert int(marg.max()) > 2 ** 39
    lmp = torch.as_tensor(rng.normal(-4.0, 0.5, 5), device=dev)
    q = [0.05, 0.5, 0.95]
    got = hitmap.moments(marg, lmp, 2.3, q)
    import line_products_reference
    want = line_products_reference.moments_torch(marg, lmp, 2.3, q)
    assert torch.equal(got["total"], want["total"]) and torch.equal(got["mode_idx"], want["mode_idx"]) and torch.equal(got["q_idx"], want["q_idx"])
    assert torch.allclose(got["mean"], want["mean"], rtol=0, atol=1e-12)


def _survey_arrays():
    import torch
    from geobipy_amd import hdf, line_products as lp
    a, _ = hdf.load_results(SURVEY)
    hm = torch.as_tensor(a[lp.VALUES + "/values/data"])
    W = float(a[lp.VALUES + "/mesh/y/edges/data"][-1])
    de = np.asarray(a[lp.VALUES + "/mesh/z/edges/data"], dtype=np.float64)
    N = hm.shape[0]
    lmp = torch.as_tensor(np.broadcast_to(np.asarray(a[lp.VALUES + "/mesh/y/relative_to/data"], dtype=np.float64).reshape(-1), (N,)) * lp.LN10)
    return hm, lmp.contiguous(), W, de, np.asarray(a["/data/elevation/data"], dtype=np.float64).reshape(-1)


def _check_line(got, spec_ranges, classes=None, percentiles=(5, 50, 95)):
    """The ``interval_*`` entries of ``got`` against the statement on the container's own arrays."""
    hm, lmp, W, de, _ = _survey_arrays()
    lo, hi, n_cells = spec_ranges
    assert np.array_equal(got["interval_cells"], n_cells) and got["interval_cells"].dtype == np.int32
    assert np.array_equal(got["interval_lo"], lo) and np.array_equal(got["interval_hi"], hi)
    marg = ir.marginals_numpy(hm.numpy(), lo, hi)
    assert got["interval_total"].dtype == np.int64 and np.array_equal(got["interval_total"], marg.sum(axis=1))
    import torch
    want = ir.products_torch(torch.as_tensor(marg), lmp, W, percentiles, 90.0, n_cells=n_cells)
    for k in ["median", "mode", "credible_low", "credible_high"] + ["percentile_%g" % p for p in percentiles]:
        assert np.array_equal(got["interval_" + k], want[k], equal_nan=True), k
    for k in ("mean", "credible_range"):
        assert np.array_equal(np.isnan(got["interval_" + k]), n_cells == 0), k
        assert np.nanmax(np.abs(got["interval_" + k] - want[k])) <= 1e-12, k
    for k in ("interval_entropy", "interval_s1", "interval_opacity", "interval_doi_index"):
        assert k not in got
    if classes is not None:
        c = ir.classes_torch(torch.as_tensor(marg), lmp, W, *classes)
        has = n_cells > 0
        P = got["interval_class_probability"]
        assert P.shape == (hm.shape[0], len(classes[0]), lo.shape[1]) and np.isnan(P[np.broadcast_to(~has[:, None, :], P.shape)]).all()
        mask = np.broadcast_to(has[:, None, :], P.shape)
        _same_probabilities(np.where(mask, P, 0.0), np.where(mask, c["probability"].numpy(), 0.0))
        assert got["interval_highest_marginal"].dtype == np.int32
        assert np.array_equal(got["interval_highest_marginal"][has], c["highest_marginal"].numpy()[has])
        assert np.isnan(got["interval_probability_of_highest_marginal"][~has]).all()


@pytest.mark.gpu
def test_from_results_with_intervals():
    from geobipy_amd import intervals as iv, line_products as lp
    hm, lmp, W, de, elev = _survey_arrays()
    N = hm.shape[0]
    plain = lp.from_results(SURVEY, block=3)
    edges = [-2.0, 0.0, 10.0, 30.25, 75.0, 219.75, 230.0]
    got = lp.from_results(SURVEY, block=3, intervals={"kind": "depth", "edges": edges}, classes=CLASSES)
    whole = lp.from_results(SURVEY, intervals={"kind": "depth", "edges": edges}, classes=CLASSES)
    with_classes = lp.from_results(SURVEY, block=3, classes=CLASSES)
    assert set(with_classes) < set(got) and all(k.startswith("interval_") for k in set(got) - set(with_classes))
    for k in with_classes:                                                      # the per-cell products are untouched by the intervals
        assert np.asarray(with_classes[k]).tobytes() == np.asarray(got[k]).tobytes(), k
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(whole[k]).tobytes(), k  # (the block size changes nothing)
    assert str(got["interval_kind"]) == "depth" and np.array_equal(got["interval_edges"], edges)
    r = iv.depth_ranges(de, edges)
    rr = tuple(np.broadcast_to(a, (N, a.size)) for a in r)
    assert r.n_cells[0] == 0 and r.n_cells[-1] == 1
    _check_line(got, rr, classes=CLASSES)
    assert not set(plain) & {k for k in got if k.startswith("interval_")}
    # overlapping pairs; horizons that differ from sounding to sounding; elevation under the container's (flat) surface
    pairs = [[0.0, 10.0], [5.0, 30.0], [29.9, 30.1]]
    got = lp.from_results(SURVEY, intervals={"kind": "pairs", "pairs": pairs}, percentiles=(10, 50, 90))
    r = iv.depth_pairs(de, pairs)
    _check_line(got, tuple(np.broadcast_to(a, (N, a.size)) for a in r), percentiles=(10, 50, 90))
    assert np.array_equal(got["interval_pairs"], pairs)
    top = np.stack([np.linspace(2.0, 40.0, N), np.full(N, 50.0)], axis=1)
    bottom = np.stack([np.linspace(12.0, 90.0, N), np.linspace(49.0, 120.0, N)], axis=1)
    top[3, 0] = np.nan
    got = lp.from_results(SURVEY, block=5, intervals={"kind": "horizons", "top": top, "bottom": bottom})
    r = iv.horizon_ranges(de, top, bottom)
    assert r.n_cells[3, 0] == 0 and r.n_cells[0, 1] == 0 and np.unique(r.n_cells[:, 0]).size > 3
    _check_line(got, tuple(r))
    got = lp.from_results(SURVEY, intervals={"kind": "elevation", "edges": [-300.0, -100.0, -30.0, 0.0, 20.0]})
    r = iv.elevation_ranges(elev, de, [-300.0, -100.0, -30.0, 0.0, 20.0])
    assert not elev.any() and r.n_cells[0].tolist() == [240, 140, 60, 0]
    _check_line(got, tuple(r))


@pytest.mark.gpu
def test_interval_entries_pass_on_elevation_unchanged():
    from geobipy_amd import line_products as lp
    hm, lmp, W, de, elev = _survey_arrays()
    got = lp.from_results(SURVEY, intervals={"kind": "depth", "edges": de}, classes=CLASSES)     # M == n_depth
    nz = de.size - 1
    assert got["interval_mean"].shape == got["mean"].shape == (hm.shape[0], nz)
    assert got["interval_mean"].tobytes() == got["mean"].tobytes() and got["interval_mode"].tobytes() == got["mode"].tobytes()
    assert got["interval_class_probability"].tobytes() == got["class_probability"].tobytes()
    on = lp.on_elevation(got, elev + 100.0, edges=np.arange(-130.0, 111.0, 10.0))
    assert on["mean"].shape == (hm.shape[0], 24)
    for k in got:
        if k.startswith("interval_"):
            assert np.asarray(on[k]).shape == np.asarray(got[k]).shape and np.asarray(on[k]).tobytes() == np.asarray(got[k]).tobytes(), k


def _two_lines(directory):
    """The committed line container as line 0 and a copy of it as line 1, its soundings moved and its surface raised."""
    from geobipy_amd import hdf
    first = os.path.join(str(directory), "0.0.h5")
    shutil.copy(SURVEY, first)
    arrays, _ = hdf.load_results(SURVEY)
    arrays = {k: np.array(v) for k, v in arrays.items()}
    arrays["/data/y/data"] = arrays["/data/y/data"] + 37.0 + 1.5 * np.arange(arrays["/data/y/data"].size)
    arrays["/data/x/data"] = arrays["/data/x/data"] + 4.0
    arrays["/data/elevation/data"] = arrays["/data/elevation/data"] + np.linspace(5.0, 9.0, arrays["/data/elevation/data"].size)
    second = os.path.join(str(directory), "1.0.results")
    np.savez(second + ".npz", **arrays)
    with open(second + ".attrs.json", "w") as fh:
        json.dump({}, fh)
    return first, second + ".npz"


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), tag


@pytest.mark.gpu
def test_survey_maps_of_intervals(tmp_path):
    import torch
    from geobipy_amd import gridding, line_products as lp, survey_volume as sv
    files = _two_lines(tmp_path)
    spec = {"kind": "elevation", "edges": [-150.0, -60.0, -20.0, 2.0, 6.0, 30.0]}
    prods = [lp.from_results(f, intervals=spec, classes=CLASSES) for f in files]
    dx, dy = 6.0, 4.0
    vol = sv.from_lines(str(tmp_path), dx, dy, variables=("mean", "percentile_95", "class_probability"), intervals=spec,
                        classes=CLASSES, block=3)
    plan = gridding.SibsonPlan(vol["x"], vol["y"], vol["x_edges"], vol["y_edges"])
    ny, nx = vol["y_edges"].size - 1, vol["x_edges"].size - 1
    for k in ("mean", "percentile_95"):
        cols = torch.as_tensor(np.concatenate([p["interval_" + k] for p in prods])).cuda()
        _same(vol[k], plan.apply(cols).cpu().numpy().reshape(5, ny, nx), k)
    cp = np.concatenate([p["interval_class_probability"] for p in prods])
    assert vol["class_probability"].shape == (3, 5, ny, nx)
    _same(vol["class_probability"], plan.apply(torch.as_tensor(cp.reshape(cp.shape[0], -1)).cuda()).cpu().numpy().reshape(3, 5, ny, nx), "classes")
    assert str(vol["interval_kind"]) == "elevation" and np.array_equal(vol["interval_edges"], spec["edges"])
    # the unit 2 .. 6 m: under line 0 (surface 0 m) no sounding has a cell of it, under line 1 (5 .. 9 m) all have -> NaN where line 0 contributes
    assert np.isnan(vol["mean"][3]).any() and np.isfinite(vol["mean"][3]).any() and np.isnan(vol["mean"][4]).any()
    # saved products are used only for the identical spec
    lp.save(prods[0], lp.output_path(files[0]))
    again = sv.from_lines(str(tmp_path), dx, dy, variables=("mean",), intervals=spec)
    _same(again["mean"], vol["mean"], "saved products of the same spec")
    lp.save(lp.from_results(files[0], intervals=spec), lp.output_path(files[0]))                   # the same spec, but no classes on file
    _same(sv.from_lines(str(tmp_path), dx, dy, variables=("class_probability",), intervals=spec, classes=CLASSES)["class_probability"],
          vol["class_probability"], "a saved file without the variable: computed from the container")
    other = {"kind": "elevation", "edges": [-150.0, -60.0, -20.0, 2.0, 6.0, 31.0]}
    fresh = sv.from_lines(str(tmp_path), dx, dy, variables=("mean",), intervals=other)
    want = [lp.from_results(f, intervals=other) for f in files]
    _same(fresh["mean"], plan.apply(torch.as_tensor(np.concatenate([p["interval_mean"] for p in want])).cuda()).cpu().numpy().reshape(5, ny, nx),
          "another spec: computed from the container")
    plain = sv.from_lines(str(tmp_path), dx, dy, variables=("mean",), depth=7)                     # (the saved file still serves the depth cells)
    assert plain["mean"].shape == (ny, nx)
    with pytest.raises(ValueError, match="units"):
        sv.from_lines(str(tmp_path), dx, dy, variables=("interval_mean",))
    with pytest.raises(ValueError, match="interval_nothing"):
        sv.from_lines(str(tmp_path), dx, dy, variables=("nothing",), intervals=spec)
    # files
    out = tmp_path / "maps"
    sv.from_lines(str(tmp_path), dx, dy, variables=("mean",), intervals=spec, out=str(out))
    assert sorted(os.listdir(str(out))) == ["survey_volume.intervals.mean.npy", "survey_volume.intervals.npz"]
    _same(np.load(sv.intervals_volume_path(str(out), "mean")), vol["mean"], "the file")
    axes = dict(np.load(str(out / sv.INTERVALS_AXES_FILE)))
    assert str(axes["interval_kind"]) == "elevation" and np.array_equal(axes["interval_edges"], spec["edges"])


@pytest.mark.gpu
def test_command_lines_write_interval_products(tmp_path):
    from geobipy_amd import intervals as iv, line_products as lp, survey_volume as sv
    files = _two_lines(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.line_products", files[0], "--depth-intervals", "0", "10", "30", "75",
                        "--class-means", "-2.5", "-1.5", "-0.5", "--class-scales", "0.3", "0.3", "0.4"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = dict(np.load(lp.output_path(files[0])))
    want = lp.from_results(files[0], intervals={"kind": "depth", "edges": [0.0, 10.0, 30.0, 75.0]}, classes=CLASSES)
    assert set(got) == set(want)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert got["interval_mean"].shape == (8, 3) and got["interval_class_probability"].shape == (8, 3, 3)
    assert got["interval_cells"].tolist() == [[20, 40, 90]] * 8
    out = tmp_path / "maps"
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--variables", "mean", "median",
                        "--elevation-intervals", "-100", "-30", "0", "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr
    vol = sv.from_lines(str(tmp_path), 6.0, 4.0, variables=("mean", "median"), intervals={"kind": "elevation", "edges": [-100.0, -30.0, 0.0]})
    for k in ("mean", "median"):
        _same(np.load(sv.intervals_volume_path(str(out), k)), vol[k], k)
        assert vol[k].shape[0] == 2 and np.isfinite(vol[k]).any()
    axes = dict(np.load(str(out / sv.INTERVALS_AXES_FILE)))
    assert axes["interval_edges"].tolist() == [-100.0, -30.0, 0.0] and list(axes["variables"]) == ["mean", "median"]
    assert not os.path.exists(str(out / sv.AXES_FILE))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--depth-intervals", "0", "10",
                        "--depth", "5"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 2 and "exclude" in r.stderr
