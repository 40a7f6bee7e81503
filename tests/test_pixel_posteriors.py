"""Pixel posteriors, CPU tier (geobipy_amd/pixel_posteriors.py, ``SibsonPlan.pool``, csrc/gbp_grid.h k_sibson_pool): the host statement of
the rule, ``pool_reference``, on a case small enough to work out by hand, its identity, its rounding and its mask; ``at``; the
argument checks of the Python entries and their refusal of host tensors; the command line; the C entry's refusals that need no device.
The kernel is held to ``pool_reference`` in tests/test_pixel_posteriors_gpu.py."""
import ctypes

import numpy as np
import pytest

import sibson_reference as sr

# two soundings on a raster of 3 x 2 pixels, in pixel coordinates: s0 on node (0, 0), s1 on node (2, 1)
PX, PY, NX, NY = np.array([0.0, 2.0]), np.array([0.0, 1.0]), 3, 2
M0 = np.array([[1, 0], [2, 1], [3, 0], [4, 2]], dtype=np.int32)               # [n_value 4, n_depth 2]
M1 = np.array([[10, 5], [20, 0], [30, 7], [40, 1]], dtype=np.int32)
MAPS = np.stack([M0, M1])
ALL = np.arange(6)


def _plan():
    index, D = sr.nearest(PX, PY, NX, NY)
    dest, src = sr.cover(D)
    return index, D, dest, src


def _lists(index, dest, src):
    return [index.reshape(-1)[src[dest == p]].tolist() for p in range(index.size)]


def test_the_hand_made_plan_is_what_the_hand_worked_out():
    index, D, dest, src = _plan()
    assert index.tolist() == [[0, 0, 1], [0, 1, 1]] and D.tolist() == [[0, 1, 1], [1, 1, 0]]
    assert _lists(index, dest, src) == [[0, 0], [0, 1, 1], [1], [0, 1], [1], []]


def test_pool_reference_by_hand():
    from geobipy_amd import pixel_posteriors as pp
    index, D, dest, src = _plan()
    Z = np.zeros_like(M0)
    # no shifts: the plain sums of the lists
    pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, ALL)
    assert pooled.dtype == np.int32 and clipped.dtype == np.int64 and pooled.shape == (6, 4, 2) and clipped.shape == (6, 2)
    for got, want in zip(pooled, (2 * M0, M0 + 2 * M1, M1, M0 + M1, M1, Z)):
        assert np.array_equal(got, want)
    assert not clipped.any()
    # s1 is one cell up the axis: where s0 is the nearest sounding (pixels 1 and 3) s1's rows move by + 1 and its last row is clipped;
    # where s1 is the nearest (pixels 2 and 4) its own counts stay where they are
    pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, ALL, u=np.array([0.0, 1.0]))
    want = (2 * M0, [[1, 0], [22, 11], [43, 0], [64, 16]], M1, [[1, 0], [12, 6], [23, 0], [34, 9]], M1, Z)
    for got, w in zip(pooled, want):
        assert np.array_equal(got, np.asarray(w))
    assert clipped.tolist() == [[0, 0], [80, 2], [0, 0], [40, 1], [0, 0], [0, 0]]
    # the other way: s1 one cell down, its first row is clipped
    pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, ALL, u=np.array([1.0, 0.0]))
    assert pooled[3].tolist() == [[21, 0], [32, 8], [43, 1], [4, 2]] and clipped[3].tolist() == [10, 5]
    assert np.array_equal(pooled[4], M1) and not clipped[4].any()
    # s1 far beyond the axis (the difference clamps to n_value): all of it is clipped, twice in pixel 1, once in pixel 3
    for far in (9.0, -4.0, 1e300):
        pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, ALL, u=np.array([0.0, far]))
        assert np.array_equal(pooled[1], M0) and np.array_equal(pooled[3], M0) and np.array_equal(pooled[2], M1)
        assert clipped.tolist() == [[0, 0], [200, 26], [0, 0], [100, 13], [0, 0], [0, 0]]


def test_ties_round_to_even():
    from geobipy_amd import pixel_posteriors as pp
    index, D, dest, src = _plan()
    shifted = lambda d: np.concatenate([np.zeros((d, 2), dtype=np.int32), M1[:4 - d]]) if d >= 0 else \
        np.concatenate([M1[-d:], np.zeros((-d, 2), dtype=np.int32)])          # noqa: E731
    for diff, d in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (0.5000000000000001, 1), (1.4999999999999998, 1)):
        pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, [3], u=np.array([0.0, diff]))
        assert np.array_equal(pooled[0], M0 + shifted(d)), (diff, d)
        assert clipped[0].tolist() == (M1.sum(0) - shifted(d).sum(0)).tolist()


def test_identity_on_a_random_case():
    from geobipy_amd import pixel_posteriors as pp
    rng = np.random.default_rng(3)
    N, nx, ny, nv, nz = 9, 8, 7, 6, 5
    index, D = sr.nearest(rng.uniform(0, nx, N), rng.uniform(0, ny, N), nx, ny)
    dest, src = sr.cover(D)
    maps = rng.integers(0, 50, (N, nv, nz)).astype(np.int32)
    maps[2] = 0
    maps[:, :, 1] = 0
    u = rng.uniform(-3.0, 3.0, N)
    u[5] = 40.0
    pixels = rng.permutation(nx * ny)
    pooled, clipped = pp.pool_reference(index, D, dest, src, maps, pixels, u=u)
    assert clipped.max() > 0 and pooled.max() > 0
    sums = maps.sum(axis=1, dtype=np.int64)                                   # [N, n_depth]
    for i, p in enumerate(pixels):
        want = sums[index.reshape(-1)[src[dest == p]]].sum(axis=0)
        assert np.array_equal(pooled[i].sum(axis=0, dtype=np.int64) + clipped[i], want)


def test_mask_repeats_and_order():
    from geobipy_amd import pixel_posteriors as pp
    index, D, dest, src = _plan()
    u = np.array([0.0, 1.0])
    whole = pp.pool_reference(index, D, dest, src, MAPS, ALL, u=u)
    # D^2 + 0.25 > 0.5 masks every pixel with D >= 1: pixel 0 (D = 0, list [s0, s0]) stays, pixel 5 has an empty list anyway
    pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, ALL, u=u, max_distance_px2=0.5)
    assert np.array_equal(pooled[0], 2 * M0) and not pooled[1:].any() and not clipped.any()
    pixels = [5, 3, 3, 0, 1, 3]
    pooled, clipped = pp.pool_reference(index, D, dest, src, MAPS, pixels, u=u)
    assert np.array_equal(pooled, whole[0][pixels]) and np.array_equal(clipped, whole[1][pixels])
    one = pp.pool_reference(index, D, dest, src, MAPS, [1], u=u)
    assert np.array_equal(one[0][0], whole[0][1]) and one[1].shape == (1, 2)
    with pytest.raises(ValueError):
        pp.pool_reference(index, D, dest, src, MAPS, [6])


def _fake_plan(n_soundings=2, nx=NX, ny=NY):
    from geobipy_amd import gridding
    plan = object.__new__(gridding.SibsonPlan)
    plan.n_soundings, plan.nx, plan.ny = n_soundings, nx, ny
    plan.x_edges, plan.y_edges = 100.0 + 10.0 * np.arange(nx + 1), -40.0 + 20.0 * np.arange(ny + 1)
    return plan


def test_at():
    from geobipy_amd import pixel_posteriors as pp
    plan = _fake_plan()
    assert pp.at(plan, 100.0, -40.0).tolist() == [0]                          # the first node
    assert pp.at(plan, [110.0, 120.0], [-20.0, -20.0]).tolist() == [4, 5]     # nodes hold their own pixel
    assert pp.at(plan, [104.9, 119.99, 129.99], [-39.0, -20.01, -0.01]).tolist() == [0, 1, 5]       # cell interiors
    assert pp.at(plan, np.array([125.0]), np.array([-30.0])).dtype == np.int64
    for x, y in ((99.99, -30.0), (130.0, -30.0), (110.0, 0.0), (110.0, -40.01), (float("nan"), -30.0)):
        with pytest.raises(ValueError):
            pp.at(plan, x, y)


def test_python_entries_refuse_bad_input_and_host_tensors():
    import torch
    from geobipy_amd import _lib, pixel_posteriors as pp
    plan = _fake_plan()
    maps = torch.as_tensor(MAPS)
    lmp = np.array([-2.0, -2.5])
    with pytest.raises(TypeError, match="gbp_sibson_pool"):
        plan.pool(maps.long())
    with pytest.raises(TypeError):
        plan.pool(MAPS)
    with pytest.raises(TypeError):
        plan.pool(maps[0])
    with pytest.raises(ValueError):
        plan.pool(maps[:1])                                                    # one map for two soundings
    with pytest.raises(ValueError):
        plan.pool(maps.transpose(1, 2))                                        # not contiguous
    with pytest.raises(ValueError, match="gbp_sibson_pool"):
        plan.pool(maps, pixels=[0, 6])
    with pytest.raises(ValueError):
        plan.pool(maps, pixels=[-1])
    with pytest.raises(TypeError):
        plan.pool(maps, pixels=[0.5])
    with pytest.raises(TypeError):
        plan.pool(maps, pixels=[[0, 1]])
    with pytest.raises(ValueError, match="together"):
        plan.pool(maps, log_mean_prior=lmp)
    with pytest.raises(ValueError, match="together"):
        plan.pool(maps, half_width=2.0)
    for bad in (np.array([-2.0, np.nan]), np.array([np.inf, 0.0]), np.array([-2.0]), np.zeros((2, 1))):
        with pytest.raises(ValueError):
            plan.pool(maps, log_mean_prior=bad, half_width=2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            plan.pool(maps, log_mean_prior=lmp, half_width=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError):
            plan.pool(maps, max_total=bad)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_sibson_pool"):
        plan.pool(maps)                                                        # everything in order, but on the host
    with pytest.raises(_lib.NativeLibraryError):
        plan.pool(maps, pixels=[1, 1, 0], log_mean_prior=lmp, half_width=2.0, max_total=100)
    with pytest.raises(ValueError):
        pp.products(plan, maps, None, None)
    with pytest.raises(ValueError):
        pp.products(plan, maps, lmp, 2.0, block=0)
    with pytest.raises(ValueError):
        pp.products(plan, maps, lmp, 2.0, percentiles=(0.0,))
    with pytest.raises(ValueError):
        pp.products(plan, maps, lmp, 2.0, percentiles=(1, 2, 3, 4, 6, 7, 8, 9))     # more quantiles than one pass holds
    with pytest.raises(ValueError):
        pp.products(plan, maps, lmp, 2.0, classes=([0.0, 1.0], [1.0]))
    with pytest.raises(ValueError):
        pp.products(plan, maps, lmp, 2.0, pixels=[7])
    with pytest.raises(TypeError):
        pp.products(plan, maps.long(), lmp, 2.0)
    with pytest.raises(_lib.NativeLibraryError):
        pp.products(plan, maps, lmp, 2.0, classes=([0.0, 1.0], [1.0, 1.0]))


def test_axis_offsets_are_numpys():
    from geobipy_amd import gridding
    from geobipy_amd.line_products import LN10
    lmp = np.array([-4.0, -3.3, 0.7])
    assert np.array_equal(gridding.axis_offsets(lmp, 2.5, 250), (lmp / LN10) / (2.0 * 2.5 / 250))


def test_command_line_arguments():
    from geobipy_amd import survey_volume as sv
    base = ["dir", "--dx", "5", "--dy", "5"]
    assert sv.parse_args(base).pooled is False
    a = sv.parse_args(base + ["--pooled", "--variables", "median", "percentile_95", "clipped_share", "--depth-cells", "2", "4", "--block", "100"])
    assert a.pooled is True and a.variables == ["median", "percentile_95", "clipped_share"] and a.depth_cells == [2, 4] and a.block == 100
    assert sv.parse_args(base + ["--pooled", "--depth", "3.5", "--mask", "40"]).depth == 3.5
    for bad in (["--elevation-axis", "2"], ["--elevation", "10"], ["--depth-intervals", "0", "5", "10"], ["--elevation-intervals", "0", "5"],
                ["--variables", "opacity"], ["--variables", "interface_probability"], ["--variables", "percentile_"],
                ["--variables", "percentile_100"], ["--variables", "percentile_5.0"], ["--variables", "class_probability"]):
        with pytest.raises(SystemExit):
            sv.parse_args(base + ["--pooled"] + bad)
    assert sv.parse_args(base + ["--variables", "opacity"]).variables == ["opacity"]        # (gridded as before)
    names, pct = sv.pooled_variables(["mean", "percentile_5", "percentile_97.5", "entropy"])
    assert names == ["mean", "percentile_5", "percentile_97.5", "entropy"] and pct == (5.0, 97.5)
    assert sv.pooled_variables(["class_probability", "highest_marginal"], classes=([0.0], [1.0]))[0] == ["class_probability", "highest_marginal"]
    with pytest.raises(ValueError, match="doi_depth"):
        sv.pooled_variables(["mean", "doi_depth"])
    with pytest.raises(ValueError, match="pooled"):
        sv.from_lines("nowhere", 5.0, 5.0, pooled=True, elevation=3.0)
    with pytest.raises(ValueError, match="pooled"):
        sv.from_lines("nowhere", 5.0, 5.0, pooled=True, elevation_edges=[0.0, 1.0])
    with pytest.raises(ValueError, match="pooled"):
        sv.from_lines("nowhere", 5.0, 5.0, pooled=True, intervals=dict(kind="depth", edges=[0.0, 5.0]))
    with pytest.raises(ValueError, match="opacity"):
        sv.from_lines("nowhere", 5.0, 5.0, pooled=True, variables=("opacity",))
    assert sv.pooled_volume_path("d", "median").endswith("survey_volume.pooled.median.npy")


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

    def call(plan=None, n=3, pixels=p, nv=4, nz=2, maps=p, u=None, max_total=10, pooled=p, clipped=p):
        return lib.gbp_sibson_pool(plan, n, pixels, nv, nz, maps, u, max_total, pooled, clipped, None)

    # every one of these is refused before anything touches a device
    assert call() == INVALID                                                   # no plan
    assert b"gbp_sibson_pool" in lib.gbp_last_error() and b"plan" in lib.gbp_last_error()
    assert call(n=-1) == INVALID and b"gbp_sibson_pool" in lib.gbp_last_error() and b"n_pixels" in lib.gbp_last_error()
    assert call(nv=0) == INVALID and call(nv=-2) == INVALID and call(nz=0) == INVALID and call(nz=-1) == INVALID
    assert b"gbp_sibson_pool" in lib.gbp_last_error() and b"n_depth" in lib.gbp_last_error()
    assert call(nz=(1 << 29) + 1) == INVALID
    assert call(max_total=-1) == INVALID and b"max_total" in lib.gbp_last_error()
    assert call(n=0, pixels=None, maps=None, pooled=None, clipped=None) == 0   # no pixels: no launch, whatever the pointers
    assert call(n=0, nv=0) == INVALID                                          # (the sizes are still checked)
