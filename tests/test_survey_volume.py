"""Survey volumes: discrete Sibson gridding of line products (csrc/gbp_grid.h, geobipy_amd/gridding.py, geobipy_amd/survey_volume.py).

(i) CPU tier: the numpy / torch statement of the algorithm (tests/sibson_reference.py) against the imported REFERENCE's own
``interpolation.sibson`` (tests/golden/make_sibson.py -> sibson.npz), EXACTLY (``==``, NaN for NaN) in values, ``index``, ``D`` and ``n``;
``centred_grid_nodes`` against the edges recorded from the reference's; the refusals of the Python entries and of the C ABI; the
command line's arguments.
(ii) GPU tier: the plan and ``apply`` against the fixture and against the formulation on shapes the fixture cannot hold, exactly again
(the device adds in the reference's order, in fp64, without FMA; the geometry is the same fp64 expression with a correctly rounded
square root): every pixel, every column, nothing excused.  One plan serving many applies and streams, banded plans, and the survey
driver and command line end to end on containers of two lines.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sibson_reference as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sibson.npz")
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")
CASES = ("centred", "cloud", "five", "lines", "masked", "single")


def _case(f, c):
    md = float(f[c + "_max_distance"])
    return dict(x=f[c + "_x"], y=f[c + "_y"], values=f[c + "_values"], x_edges=f[c + "_x_edges"], y_edges=f[c + "_y_edges"],
                max_distance=None if np.isinf(md) else md, out=f[c + "_out"], index=f[c + "_index"], D=f[c + "_D"], n=f[c + "_n"])


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    assert bad.size == 0, (tag, "first differing entries", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_fixture_holds_the_cases_the_issue_names():
    f = np.load(GOLDEN)
    assert tuple(f["cases"]) == CASES
    c = _case(f, "lines")
    assert (c["D"] == 0).sum() == 1 and np.isnan(c["values"]).sum() == 1
    assert c["x"].max() > c["x_edges"][-1]                                    # a sounding outside the grid
    assert np.diff(c["x_edges"])[0] == 16.0 and np.diff(c["y_edges"])[0] == 32.0
    m = _case(f, "masked")
    assert np.isnan(m["out"]).sum() > np.isnan(c["out"]).sum() and not np.isnan(m["out"]).all()
    assert _case(f, "single")["x"].size == 1 and _case(f, "five")["n"].max() > 400
    assert _case(f, "cloud")["values"].shape == (60, 3) and _case(f, "cloud")["n"].shape == (12, 17)


@pytest.mark.parametrize("name", CASES)
def test_formulation_equals_the_reference(name):
    c = _case(np.load(GOLDEN), name)
    out, index, D, n = sr.sibson(c["x"], c["y"], c["values"], c["x_edges"], c["y_edges"], c["max_distance"])
    _same(index, c["index"], name + " index")
    _same(D, c["D"], name + " D")
    _same(n, c["n"], name + " n")
    _same(out, c["out"], name + " values")


def test_centred_grid_nodes_equal_the_reference():
    from geobipy_amd import gridding
    f = np.load(GOLDEN)
    b, s = f["centred_bounds"], f["centred_spacing"]
    _same(gridding.centred_grid_nodes(b[:2], s[0]), f["centred_x_edges"], "x edges")
    _same(gridding.centred_grid_nodes(b[2:], s[1]), f["centred_y_edges"], "y edges")
    xe, ye = gridding.centred_mesh(f["centred_x"], f["centred_y"], s[0], s[1])
    _same(xe, f["centred_x_edges"], "mesh x")
    _same(ye, f["centred_y_edges"], "mesh y")
    one = gridding.centred_grid_nodes((7.0, 7.0), 4.0)                         # every sounding on one y: one row of pixels
    assert one.tolist() == [5.0, 9.0]
    with pytest.raises(ValueError):
        gridding.centred_grid_nodes((0.0, 1.0), 0.0)
    px, py, dx, dy = gridding.pixel_coordinates(f["lines_x"], f["lines_y"], f["lines_x_edges"], f["lines_y_edges"])
    rx, ry, rdx, rdy = sr.pixel_coordinates(f["lines_x"], f["lines_y"], f["lines_x_edges"], f["lines_y_edges"])
    _same(px, rx, "px")
    _same(py, ry, "py")
    assert (dx, dy) == (rdx, rdy) == (16.0, 32.0)


def test_python_entries_refuse_bad_input_and_host_tensors():
    import torch
    from geobipy_amd import _lib, gridding
    x, y = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0])
    e = np.arange(6.0)
    with pytest.raises(ValueError):
        gridding.pixel_coordinates(x, y, np.array([0.0, 1.0, 2.5, 3.0]), e)   # non-uniform
    with pytest.raises(ValueError):
        gridding.pixel_coordinates(x, y, e, e[::-1])                            # decreasing
    with pytest.raises(ValueError):
        gridding.pixel_coordinates(x, y, e[:1], e)                              # no pixel
    with pytest.raises(ValueError):
        gridding.pixel_coordinates(x, y[:2], e, e)                              # mismatched soundings
    with pytest.raises(ValueError):
        gridding.pixel_coordinates(x[:0], y[:0], e, e)
    with pytest.raises(_lib.NativeLibraryError):
        gridding.SibsonPlan(x, y, e, e, device="cpu")
    with pytest.raises(_lib.NativeLibraryError):
        gridding.sibson(x, y, torch.zeros(3, dtype=torch.float64), e, e)
    with pytest.raises(_lib.NativeLibraryError):
        gridding.sibson(x, y, np.zeros(3), e, e)
    with pytest.raises(_lib.NativeLibraryError):
        gridding.SibsonPlan.apply(object.__new__(gridding.SibsonPlan), torch.zeros(3, dtype=torch.float64))


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
    inf = float("inf")

    def create(N=4, px=p, py=p, nx=5, ny=6, md=inf, budget=None, out=True):
        h = ctypes.c_void_p()
        o = ctypes.byref(h) if out else None
        if budget is None:
            rc = lib.gbp_sibson_plan_create(N, px, py, nx, ny, md, None, o)
        else:
            rc = lib.gbp_sibson_plan_create_ex(N, px, py, nx, ny, md, budget, None, o)
        assert not h.value
        return rc

    # every one of these is refused before anything touches a device
    assert create(N=0) == INVALID and create(N=-2) == INVALID
    assert b"gbp_sibson_plan_create" in lib.gbp_last_error()
    assert create(nx=0) == INVALID and create(ny=0) == INVALID and create(nx=-1) == INVALID
    assert create(px=None) == INVALID and create(py=None) == INVALID
    assert create(out=False) == INVALID
    assert create(nx=1 << 16, ny=1 << 15) == INVALID                           # nx * ny beyond int32
    assert b"gbp_sibson_plan_create" in lib.gbp_last_error() and b"range" in lib.gbp_last_error()
    assert create(md=float("nan")) == INVALID
    assert create(budget=-1) == INVALID
    assert b"gbp_sibson_plan_create" in lib.gbp_last_error()
    assert lib.gbp_sibson_apply(None, 3, p, p, None) == INVALID
    assert b"gbp_sibson_apply" in lib.gbp_last_error()
    assert lib.gbp_sibson_plan_query(None, None, None, None, None, None) == INVALID
    assert b"gbp_sibson_plan_query" in lib.gbp_last_error()
    lib.gbp_sibson_plan_destroy(None)                                          # a no-op


def test_command_line_arguments():
    from geobipy_amd import survey_volume as sv
    a = sv.parse_args(["dir", "--dx", "50", "--dy", "100"])
    assert (a.dx, a.dy, a.variables, a.mask, a.depth, a.depth_cells) == (50.0, 100.0, ["mean"], None, None, None)
    a = sv.parse_args(["dir", "--dx", "50", "--dy", "100", "--variables", "mean", "percentile_5", "--mask", "300", "--depth", "12.5",
                       "--device", "cuda:0"])
    assert a.variables == ["mean", "percentile_5"] and a.mask == 300.0 and a.depth == 12.5 and a.device == "cuda:0"
    assert sv.parse_args(["dir", "--dx", "5", "--dy", "5", "--depth-cells", "3", "9"]).depth_cells == [3, 9]
    for bad in (["dir"], ["dir", "--dx", "50"], ["--dx", "5", "--dy", "5"], ["dir", "--dx", "0", "--dy", "5"],
                ["dir", "--dx", "5", "--dy", "-1"], ["dir", "--dx", "nan", "--dy", "5"], ["dir", "--dx", "5", "--dy", "5", "--mask", "0"],
                ["dir", "--dx", "5", "--dy", "5", "--depth", "3", "--depth-cells", "1", "2"],
                ["dir", "--dx", "5", "--dy", "5", "--depth-cells", "4", "2"], ["dir", "--dx", "5", "--dy", "5", "--depth-cells", "-1", "2"],
                ["dir", "--dx", "5", "--dy", "5", "--block", "0"], ["dir", "--dx", "5", "--dy", "5", "--variables", "mean", "mean"]):
        with pytest.raises(SystemExit):
            sv.parse_args(bad)
    e = np.arange(11.0) * 2.0
    assert sv.depth_cells(None, e) == slice(0, 10) and sv.depth_cells(3, e) == slice(3, 4) and sv.depth_cells(3.0, e) == slice(1, 2)
    assert sv.depth_cells((2, 5), e) == slice(2, 6) and sv.depth_cells((9.0, 2.0), e) == slice(1, 5)
    assert sv.depth_cells(slice(4, 7), e) == slice(4, 7, 1)
    for bad in (10, 20.0, -0.1, (1, 2, 3)):
        with pytest.raises(ValueError):
            sv.depth_cells(bad, e)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU

def _plan_equals(plan, index, D, n, tag):
    _same(plan.index.cpu().numpy(), index, tag + " index")
    got = plan.distance.cpu().numpy()
    bad = np.argwhere(got != D)
    assert bad.size == 0, (tag, "D differs at pixels", bad[:5].tolist(), "device", got[tuple(bad[0])], "formulation", D[tuple(bad[0])])
    _same(plan.count.cpu().numpy(), n, tag + " n")
    assert plan.list_length == int(n.sum()) and plan.longest_list == int(n.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_plan_and_apply_equal_the_reference(name):
    import torch
    from geobipy_amd import gridding
    c = _case(np.load(GOLDEN), name)
    plan = gridding.SibsonPlan(c["x"], c["y"], c["x_edges"], c["y_edges"], max_distance=c["max_distance"])
    _plan_equals(plan, c["index"], c["D"], c["n"], name)
    v = torch.as_tensor(c["values"]).cuda()
    _same(plan.apply(v).cpu().numpy(), c["out"], name + " values")
    for col in range(v.shape[1]):                                              # a single column, as the reference takes it
        _same(plan.apply(v[:, col].contiguous()).cpu().numpy(), c["out"][col], "%s column %d" % (name, col))
    _same(gridding.sibson(c["x"], c["y"], v, c["x_edges"], c["y_edges"], c["max_distance"]).cpu().numpy(), c["out"], name + " sibson()")


def _soundings(kind, N, nx, ny, rng, dx, dy):
    if kind == "cloud":
        return rng.uniform(-0.03 * nx * dx, 1.03 * nx * dx, N), rng.uniform(0.0, ny * dy, N)
    n_lines = max(1, min(N, int(round(np.sqrt(N / 8.0)))))                      # flight lines along x, jittered
    line = np.arange(N) % n_lines
    along = (np.arange(N) // n_lines + rng.uniform(-0.2, 0.2, N)) / max(1, (N - 1) // n_lines + 1)
    return along * nx * dx, ((line + 0.5) / n_lines + rng.uniform(-0.1, 0.1, N) / n_lines) * ny * dy


SHAPES = [  # kind, N, nx, ny, C, mask (in pixels squared; None: no mask), a NaN column
    ("cloud", 1, 50, 40, 1, None, False),
    ("cloud", 7, 64, 33, 63, 30.0, False),
    ("lines", 300, 120, 90, 1320, None, False),
    ("cloud", 5000, 300, 280, 64, None, True),
    ("lines", 20000, 300, 300, 65, 3.0, False),
    ("lines", 800, 100, 1, 440, None, True),
    ("cloud", 2000, 33, 257, 440, 12.0, False),
    ("lines", 64, 97, 31, 129, None, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,nx,ny,C,mask,nan_column", SHAPES)
def test_kernels_equal_the_formulation(kind, N, nx, ny, C, mask, nan_column):
    import torch
    from geobipy_amd import gridding
    rng = np.random.default_rng(N * 7 + C)
    dx, dy = 12.5, 40.0
    x, y = _soundings(kind, N, nx, ny, rng, dx, dy)
    if ny == 1:
        y = np.full(N, 3.0)
    xe, ye = 1000.0 + dx * np.arange(nx + 1), -500.0 + dy * np.arange(ny + 1)
    x, y = x + xe[0], y + ye[0]
    v = rng.normal(size=(N, C))
    if nan_column:
        v[:, C // 2] = np.nan
        v[rng.integers(N), 0] = np.nan
    md = None if mask is None else mask * dx * dy
    want, index, D, n = sr.sibson(x, y, v, xe, ye, md)
    plan = gridding.SibsonPlan(x, y, xe, ye, max_distance=md)
    tag = "%s N=%d %dx%d C=%d" % (kind, N, nx, ny, C)
    _plan_equals(plan, index, D, n, tag)
    print(tag, "lists: total %d longest %d median %d; NaN pixels %d" % (plan.list_length, plan.longest_list, int(np.median(n)),
                                                                        int(np.isnan(want[0]).sum())))
    _same(plan.apply(torch.as_tensor(v).cuda()).cpu().numpy(), want, tag)


@pytest.mark.gpu
def test_one_plan_serves_many_applies_and_streams():
    import torch
    from geobipy_amd import gridding
    rng = np.random.default_rng(5)
    N, nx, ny = 900, 140, 75
    x, y = _soundings("lines", N, nx, ny, rng, 10.0, 10.0)
    xe, ye = 10.0 * np.arange(nx + 1), 10.0 * np.arange(ny + 1)
    a, b = torch.as_tensor(rng.normal(size=(N, 70))).cuda(), torch.as_tensor(rng.normal(size=(N, 3))).cuda()
    plan = gridding.SibsonPlan(x, y, xe, ye, max_distance=900.0)
    first = plan.apply(a).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = plan.apply(b)
        again = plan.apply(a)
    side.synchronize()
    _same(again.cpu().numpy(), first, "the same input twice, on another stream")
    _same(gridding.SibsonPlan(x, y, xe, ye, max_distance=900.0).apply(a).cpu().numpy(), first, "a fresh plan, first values")
    _same(gridding.SibsonPlan(x, y, xe, ye, max_distance=900.0).apply(b).cpu().numpy(), second.cpu().numpy(), "a fresh plan, second values")
    for _ in range(3):
        _same(plan.apply(a).cpu().numpy(), first, "repeat")


@pytest.mark.gpu
def test_banded_plans_give_the_same_bits():
    import torch
    from geobipy_amd import _lib, gridding
    rng = np.random.default_rng(6)
    N, nx, ny = 40, 90, 70
    x, y = _soundings("cloud", N, nx, ny, rng, 10.0, 10.0)
    xe, ye = 10.0 * np.arange(nx + 1), 10.0 * np.arange(ny + 1)
    v = torch.as_tensor(rng.normal(size=(N, 66))).cuda()
    whole = gridding.SibsonPlan(x, y, xe, ye)
    assert whole.n_bands == 1
    want = whole.apply(v).cpu().numpy()
    row = int(whole.count.sum(dim=1).max())                                     # the longest destination row's lists
    for budget in (4 * row, 4 * (2 * row + 1), whole.list_length * 4 // 3):
        banded = gridding.SibsonPlan(x, y, xe, ye, list_budget_bytes=budget)
        assert banded.n_bands > 1 and banded.bytes_held < whole.bytes_held
        _same(banded.count.cpu().numpy(), whole.count.cpu().numpy(), "n")
        _same(banded.apply(v).cpu().numpy(), want, "budget %d: %d bands" % (budget, banded.n_bands))
        _same(banded.apply(v[:, :2].contiguous()).cpu().numpy(), want[:2], "a second apply of a banded plan")
    with pytest.raises(_lib.NativeLibraryError, match="gbp_sibson_plan_create"):
        gridding.SibsonPlan(x, y, xe, ye, list_budget_bytes=4 * (row - 1))


@pytest.mark.gpu
def test_c_abi_refusals_on_the_device():
    import torch
    from geobipy_amd import _lib, gridding
    lib = _lib.load()
    px = torch.tensor([1.0, float("nan"), 2.0], dtype=torch.float64).cuda()
    py = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64).cuda()
    h = ctypes.c_void_p()
    assert lib.gbp_sibson_plan_create(3, px.data_ptr(), py.data_ptr(), 4, 4, float("inf"), None, ctypes.byref(h)) == -1 and not h.value
    assert b"gbp_sibson_plan_create" in lib.gbp_last_error() and b"non-finite" in lib.gbp_last_error()
    far = py * float("inf")
    assert lib.gbp_sibson_plan_create(3, py.data_ptr(), far.data_ptr(), 4, 4, float("inf"), None, ctypes.byref(h)) == -1 and not h.value
    plan = gridding.SibsonPlan([1.0, 2.0], [1.0, 2.0], np.arange(5.0), np.arange(4.0))
    v, out = torch.zeros((2, 1), dtype=torch.float64).cuda(), torch.zeros((1, 3, 4), dtype=torch.float64).cuda()
    assert lib.gbp_sibson_apply(plan._handle, 0, v.data_ptr(), out.data_ptr(), None) == -1
    assert lib.gbp_sibson_apply(plan._handle, 1, None, out.data_ptr(), None) == -1
    assert lib.gbp_sibson_apply(plan._handle, 1, v.data_ptr(), None, None) == -1
    assert lib.gbp_sibson_apply(plan._handle, 1 << 23, v.data_ptr(), out.data_ptr(), None) == -1
    assert b"gbp_sibson_apply" in lib.gbp_last_error()
    for bad in (torch.zeros(3, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.float32).cuda(),
                torch.zeros((2, 0), dtype=torch.float64).cuda(), torch.zeros((2, 1, 1), dtype=torch.float64).cuda()):
        with pytest.raises(ValueError):
            plan.apply(bad)
    with pytest.raises(ValueError):
        gridding.SibsonPlan([1.0, float("inf")], [1.0, 2.0], np.arange(5.0), np.arange(4.0))
    assert plan.apply(torch.ones(2, dtype=torch.float64).cuda()).shape == (3, 4)


def _two_lines(directory):
    """The committed line container as line 0 and a copy of it as line 1 -- a stand-in container, its soundings moved in x and y."""
    from geobipy_amd import hdf
    first = os.path.join(str(directory), "0.0.h5")
    shutil.copy(SURVEY, first)
    arrays, _ = hdf.load_results(SURVEY)
    arrays = {k: np.array(v) for k, v in arrays.items()}
    arrays["/data/y/data"] = arrays["/data/y/data"] + 37.0 + 1.5 * np.arange(arrays["/data/y/data"].size)
    arrays["/data/x/data"] = arrays["/data/x/data"] + 4.0
    arrays["/data/line_number/data"] = arrays["/data/line_number/data"] + 1.0
    arrays["/data/elevation/data"] = arrays["/data/elevation/data"] + np.linspace(5.0, 9.0, arrays["/data/elevation/data"].size)
    second = os.path.join(str(directory), "1.0.results")
    np.savez(second + ".npz", **arrays)
    with open(second + ".attrs.json", "w") as fh:
        json.dump({}, fh)
    return first, second + ".npz"


@pytest.mark.gpu
def test_survey_volume_end_to_end(tmp_path):
    import torch
    from geobipy_amd import gridding, hdf, line_products as lp, survey_volume as sv
    files = _two_lines(tmp_path)
    prods = [lp.from_results(f) for f in files]
    xs = np.concatenate([np.asarray(hdf.load_results(f)[0]["/data/x/data"], dtype=np.float64) for f in files])
    ys = np.concatenate([np.asarray(hdf.load_results(f)[0]["/data/y/data"], dtype=np.float64) for f in files])
    assert xs.size == 2 * prods[0]["mean"].shape[0] and np.unique(ys).size > 2
    dx, dy = 6.0, 4.0
    xe, ye = gridding.centred_mesh(xs, ys, dx, dy)
    plan = gridding.SibsonPlan(xs, ys, xe, ye)
    want = {k: plan.apply(torch.as_tensor(np.concatenate([p[k] for p in prods])).cuda()).cpu().numpy() for k in ("mean", "percentile_95")}
    nz = prods[0]["mean"].shape[1]

    vol = sv.from_lines(str(tmp_path), dx, dy, variables=("mean", "percentile_95"), block=100)
    _same(vol["x_edges"], xe, "x edges")
    _same(vol["y_edges"], ye, "y edges")
    _same(vol["depth_edges"], prods[0]["depth_edges"], "depth edges")
    assert vol["mean"].shape == (nz, ye.size - 1, xe.size - 1)
    for k in want:
        _same(vol[k], want[k], k)
    _same(vol["count"], plan.count.cpu().numpy(), "count")
    _same(vol["nearest_distance"], plan.distance.cpu().numpy(), "nearest_distance")
    elev = np.concatenate([np.asarray(hdf.load_results(f)[0]["/data/elevation/data"], dtype=np.float64) for f in files])
    _same(vol["elevation"], plan.apply(torch.as_tensor(elev).cuda()).cpu().numpy(), "elevation")
    assert np.isfinite(vol["mean"]).any()

    one = sv.from_lines(list(files), dx, dy, depth=7)
    _same(one["mean"], vol["mean"][7], "depth cell 7")
    d = 0.5 * (prods[0]["depth_edges"][11] + prods[0]["depth_edges"][12])
    _same(sv.from_lines(str(tmp_path), dx, dy, depth=float(d))["mean"], vol["mean"][11], "the cell holding a depth")
    some = sv.from_lines(str(tmp_path), dx, dy, depth=(20, 29), max_distance=None)
    _same(some["mean"], vol["mean"][20:30], "cells 20 .. 29")
    _same(some["depth_edges"], prods[0]["depth_edges"][20:31], "their edges")
    masked = sv.from_lines(str(tmp_path), dx, dy, depth=7, max_distance=dx * dy * 2.0)
    hidden = np.isnan(masked["mean"]) & ~np.isnan(one["mean"])
    assert hidden.any() and np.array_equal(hidden, (vol["nearest_distance"].astype(np.float64) ** 2 + 0.25 > 2.0) & ~np.isnan(one["mean"]))

    # the wedge line alone: every sounding on one y, a grid of one row
    row = sv.from_lines(files[0], dx, dy, depth=7)
    assert row["mean"].shape == (1, row["x_edges"].size - 1) and row["y_edges"].size == 2 and np.isfinite(row["mean"]).any()

    # a line with another depth mesh is refused
    other = dict(np.load(files[1]))
    key = lp.VALUES + "/mesh/z/edges/data"
    other[key] = other[key] * 1.5
    np.savez(os.path.join(str(tmp_path), "2.0.results.npz"), **other)
    with open(os.path.join(str(tmp_path), "2.0.results.attrs.json"), "w") as fh:
        json.dump({}, fh)
    with pytest.raises(ValueError, match="depth mesh"):
        sv.from_lines(str(tmp_path), dx, dy, depth=7)


@pytest.mark.gpu
def test_command_line_writes_the_volumes(tmp_path):
    import torch
    from geobipy_amd import gridding, line_products as lp, survey_volume as sv
    files = _two_lines(tmp_path)
    lp.save(lp.from_results(files[0]), lp.output_path(files[0]))                # one line's products on file, the other's computed
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "volume"
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--variables", "mean",
                        "median", "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    axes = dict(np.load(str(out / sv.AXES_FILE)))
    vol = sv.from_lines(str(tmp_path), 6.0, 4.0, variables=("mean", "median"))
    for k in ("x_edges", "y_edges", "depth_edges", "elevation", "count", "nearest_distance"):
        _same(axes[k], vol[k], k)
    assert list(axes["variables"]) == ["mean", "median"]
    for k in ("mean", "median"):
        _same(np.load(sv.volume_path(str(out), k), mmap_mode="r"), vol[k], k)
    # the mean volume at a depth cell is the reference-pinned apply of that cell's line products
    prods = [lp.from_results(f) for f in files]
    plan = gridding.SibsonPlan(vol["x"], vol["y"], vol["x_edges"], vol["y_edges"])
    cell = torch.as_tensor(np.concatenate([p["mean"][:, 30] for p in prods])).cuda()
    _same(np.load(sv.volume_path(str(out), "mean"))[30], plan.apply(cell).cpu().numpy(), "cell 30")
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--depth-cells", "5", "9",
                        "--mask", "60", "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    _same(np.load(sv.volume_path(str(out), "mean")), sv.from_lines(str(tmp_path), 6.0, 4.0, depth=slice(5, 10), max_distance=60.0)["mean"], "cells 5 .. 9")
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--variables", "nothing",
                        "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 1 and "nothing" in r.stderr
