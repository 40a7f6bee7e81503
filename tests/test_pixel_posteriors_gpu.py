"""Pixel posteriors, GPU tier: k_sibson_pool (csrc/gbp_grid.h) through ``SibsonPlan.pool`` against the host statement of the rule,
``pixel_posteriors.pool_reference``, over the lists of tests/sibson_reference.py -- with ``==``: the sums are integers, so nothing is
excused -- its identity, one sounding alone, the refusals, ``pixel_posteriors.products`` block by block, and ``survey_volume``'s pooled
volumes end to end on containers of two lines."""
import ctypes
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sibson_reference as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")
DX, DY = 12.5, 40.0


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    assert bad.size == 0, (tag, "first differing entries", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """(x, y, x_edges, y_edges, index, D, dest, src) of a case's soundings and raster, the lists from the numpy formulation; shared."""
    rng = np.random.default_rng(11)
    if name == "rows":                                                         # 7 soundings in two rows on 9 x 6 pixels
        nx, ny = 9, 6
        px, py = np.array([0.6, 3.1, 5.4, 8.2, 1.7, 4.3, 7.0]), np.array([1.2, 1.1, 1.3, 1.2, 4.1, 4.2, 4.0])
    elif name == "jittered":                                                   # 40 jittered soundings on 17 x 11
        nx, ny = 17, 11
        g = np.stack(np.meshgrid(np.linspace(0.5, 16.0, 8), np.linspace(0.5, 10.0, 5)), -1).reshape(-1, 2)
        px, py = g[:, 0] + rng.uniform(-0.7, 0.7, 40), g[:, 1] + rng.uniform(-0.7, 0.7, 40)
    else:                                                                      # one sounding alone
        nx, ny = 6, 5
        px, py = np.array([2.3]), np.array([1.6])
    xe, ye = 1000.0 + DX * np.arange(nx + 1), -500.0 + DY * np.arange(ny + 1)
    x, y = xe[0] + px * DX, ye[0] + py * DY
    rpx, rpy, _, _ = sr.pixel_coordinates(x, y, xe, ye)
    index, D = sr.nearest(rpx, rpy, nx, ny)
    dest, src = sr.cover(D)
    for a in (index, D, dest, src):
        a.setflags(write=False)
    return x, y, xe, ye, index, D, dest, src


def _maps(rng, N, nv, nz):
    """Random sparse maps with an empty map (a sounding that never burned in) and a column of zeros."""
    m = (rng.integers(0, 1000, (N, nv, nz)) * (rng.random((N, nv, nz)) < 0.4)).astype(np.int32)
    if N > 2:
        m[2] = 0
    if nz > 1:
        m[:, :, nz // 2] = 0
    return m


def _prior_means(rng, N, nv, hw, index, dest, src):
    """(log_mean_prior, u as the device is given it): axis offsets whose differences between neighbours span -3 .. +3 cells, an exact
    .5 tie between soundings 0 and 1 (found by stepping the last bits of sounding 1's prior mean), a 1.5 cells elsewhere, and one
    sounding far beyond any axis."""
    from geobipy_amd import gridding
    w, ln10 = 2.0 * hw / nv, 2.302585092994046
    u = np.array([0.25, 0.75, -1.5, 1000.0, 1.0, 1.5, -1.6, 0.4, -0.3, 1.25, -1.45, 0.0, -0.8])[np.arange(N) % 13]
    u[4:] += rng.uniform(-0.05, 0.05, N)[4:]
    u[16::13] = 0.1                                                            # (one sounding only is far away)
    lmp = u * w * ln10
    flat = index.reshape(-1)
    if N > 1:
        for cand in [lmp[1]] + [np.nextafter(lmp[1], s * np.inf) for s in (1, -1)]:
            lmp[1] = cand
            u = gridding.axis_offsets(lmp, hw, nv)
            if u[1] - u[0] == 0.5:
                break
        diff = u[flat[src]] - u[flat[dest]]
        near = diff[np.abs(diff) < 100.0]
        assert set(np.rint(near)) >= set(range(-3, 4)) and (np.abs(near) == 0.5).any(), sorted(set(np.rint(near)))
    return lmp, gridding.axis_offsets(lmp, hw, nv)


SHAPES = [("rows", 10, 1), ("rows", 10, 65), ("rows", 37, 63), ("rows", 37, 130), ("rows", 131, 5),
          ("jittered", 10, 63), ("jittered", 10, 130), ("jittered", 37, 1), ("jittered", 37, 65)]


@pytest.mark.parametrize("name,nv,nz", SHAPES)
def test_kernel_equals_pool_reference(name, nv, nz):
    import torch
    from geobipy_amd import gridding, pixel_posteriors as pp
    x, y, xe, ye, index, D, dest, src = _geometry(name)
    N, P = x.size, index.size
    rng = np.random.default_rng(nv * 1000 + nz)
    maps = _maps(rng, N, nv, nz)
    hw = 0.0625 * nv                                                           # value cells of 0.125
    lmp, u = _prior_means(rng, N, nv, hw, index, dest, src)
    md = 2.0 * DX * DY                                                         # masks the pixels with D >= 2
    dmaps = torch.as_tensor(maps).cuda()
    plan = gridding.SibsonPlan(x, y, xe, ye)
    masked = gridding.SibsonPlan(x, y, xe, ye, max_distance=md)
    _same(plan.index.cpu().numpy(), index, "index")
    assert ((D.astype(np.float64) ** 2 + 0.25 > 2.0) & (masked.count.cpu().numpy() > 0)).any()
    everything = np.arange(P)
    mixed = np.concatenate([everything[::-1], [3, 3, P - 1, 0, 3]])
    tag = "%s nv=%d nz=%d" % (name, nv, nz)

    want = pp.pool_reference(index, D, dest, src, maps, everything)
    got = plan.pool(dmaps)
    _same(got["pooled"].cpu().numpy(), want[0], tag + " no shifts, pooled")
    _same(got["clipped"].cpu().numpy(), want[1], tag + " no shifts, clipped")
    assert got["log_mean_prior"] is None and not want[1].any()
    n = np.bincount(dest, minlength=P).astype(np.int32)
    _same(got["count"].cpu().numpy(), n, tag + " count")

    want = pp.pool_reference(index, D, dest, src, maps, everything, u=u)
    assert (want[1] > 0).any() and (want[0] > 0).any()
    got = plan.pool(dmaps, log_mean_prior=lmp, half_width=hw)
    _same(got["pooled"].cpu().numpy(), want[0], tag + " shifts, pooled")
    _same(got["clipped"].cpu().numpy(), want[1], tag + " shifts, clipped")
    _same(got["log_mean_prior"].cpu().numpy(), lmp[index.reshape(-1)], tag + " the pixels' axes")
    # the identity: nothing is lost between pooled and clipped
    sums = maps.sum(axis=1, dtype=np.int64)
    lists = np.zeros((P, nz), dtype=np.int64)
    np.add.at(lists, dest, sums[index.reshape(-1)[src]])
    _same(got["pooled"].sum(dim=1, dtype=torch.int64).cpu().numpy() + got["clipped"].cpu().numpy(), lists, tag + " identity")

    got = plan.pool(dmaps, pixels=mixed, log_mean_prior=torch.as_tensor(lmp), half_width=hw, max_total=int(sums.max()))
    _same(got["pooled"].cpu().numpy(), want[0][mixed], tag + " reversed with repeats, pooled")
    _same(got["clipped"].cpu().numpy(), want[1][mixed], tag + " reversed with repeats, clipped")
    got = plan.pool(dmaps, pixels=torch.tensor([P // 2]), log_mean_prior=lmp, half_width=hw)
    _same(got["pooled"].cpu().numpy(), want[0][P // 2:P // 2 + 1], tag + " one pixel, pooled")
    _same(got["clipped"].cpu().numpy(), want[1][P // 2:P // 2 + 1], tag + " one pixel, clipped")

    want = pp.pool_reference(index, D, dest, src, maps, mixed, u=u, max_distance_px2=masked.max_distance_px2)
    hidden = (D.reshape(-1).astype(np.float64) ** 2 + 0.25 > masked.max_distance_px2)[mixed]
    assert hidden.any() and not hidden.all() and not want[0][hidden].any() and want[0][~hidden].any()
    got = masked.pool(dmaps, pixels=mixed, log_mean_prior=lmp, half_width=hw)
    _same(got["pooled"].cpu().numpy(), want[0], tag + " masked, pooled")
    _same(got["clipped"].cpu().numpy(), want[1], tag + " masked, clipped")
    _same(got["count"].cpu().numpy(), np.where(hidden, 0, n[mixed]).astype(np.int32), tag + " masked, count")


def test_one_sounding_alone():
    import torch
    from geobipy_amd import gridding, hitmap
    x, y, xe, ye, index, D, dest, src = _geometry("alone")
    rng = np.random.default_rng(2)
    nv, nz = 37, 65
    maps = _maps(rng, 1, nv, nz)
    dmaps = torch.as_tensor(maps).cuda()
    lmp = torch.tensor([-3.0], dtype=torch.float64)
    plan = gridding.SibsonPlan(x, y, xe, ye)
    got = plan.pool(dmaps, log_mean_prior=lmp, half_width=2.0)
    count = got["count"].cpu().numpy()
    assert (count > 1).all()                                                   # every pixel is covered, by itself and by neighbours
    _same(got["pooled"].cpu().numpy(), count[:, None, None] * maps, "count x map")
    assert not got["clipped"].any()
    own = hitmap.moments(dmaps, lmp, 2.0, [0.5])["mode_idx"].cpu().numpy()
    mode = hitmap.moments(got["pooled"], got["log_mean_prior"], 2.0, [0.5])["mode_idx"].cpu().numpy()
    covered = count > 0
    _same(mode[covered], np.broadcast_to(own, mode.shape)[covered], "the mode is the sounding's own")


def test_refusals_on_the_device():
    import torch
    from geobipy_amd import _lib, gridding
    x, y, xe, ye, index, D, dest, src = _geometry("jittered")
    N, P = x.size, index.size
    maps = torch.ones((N, 4, 3), dtype=torch.int32).cuda()
    plan = gridding.SibsonPlan(x, y, xe, ye)
    assert plan.longest_list > 1
    fits = 0x7fffffff // plan.longest_list
    assert plan.pool(maps, max_total=fits)["pooled"].shape == (P, 4, 3)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_sibson_pool.*2\\^31"):
        plan.pool(maps, max_total=fits + 1)
    row = int(plan.count.sum(dim=1).max())
    banded = gridding.SibsonPlan(x, y, xe, ye, list_budget_bytes=4 * row)
    assert banded.n_bands > 1
    with pytest.raises(_lib.NativeLibraryError, match="gbp_sibson_pool.*banded"):
        banded.pool(maps)
    for bad in ([P], [0, -1], np.array([1 << 40])):
        with pytest.raises(ValueError, match="gbp_sibson_pool"):
            plan.pool(maps, pixels=bad)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_sibson_pool"):
        plan.pool(maps.cpu())                                                  # maps on another device
    with pytest.raises(TypeError, match="gbp_sibson_pool"):
        plan.pool(maps.long())
    with pytest.raises(TypeError, match="gbp_sibson_pool"):
        plan.pool(maps.double())
    lib = _lib.load()
    pix = torch.zeros(2, dtype=torch.int32).cuda()
    out, lost = torch.zeros((2, 4, 3), dtype=torch.int32).cuda(), torch.zeros((2, 3), dtype=torch.int64).cuda()

    def call(handle=plan._handle, n=2, pixels=pix.data_ptr(), nv=4, nz=3, m=maps.data_ptr(), max_total=4, pooled=out.data_ptr()):
        return lib.gbp_sibson_pool(handle, n, pixels, nv, nz, m, None, max_total, pooled, lost.data_ptr(), None)

    assert call(pixels=None) == -1 and call(m=None) == -1 and call(pooled=None) == -1
    assert b"gbp_sibson_pool" in lib.gbp_last_error() and b"NULL" in lib.gbp_last_error()
    assert call(handle=None) == -1 and call(nv=0) == -1 and call(n=-1) == -1 and call(max_total=-1) == -1
    assert call(handle=banded._handle) == -1 and b"banded" in lib.gbp_last_error()
    assert call(n=0) == 0 and call() == 0
    assert lib.gbp_sibson_pool(plan._handle, 2, pix.data_ptr(), 4, 3, maps.data_ptr(), None, 4, out.data_ptr(), None, None) == 0   # no clipped
    torch.cuda.synchronize()


def test_products_do_not_depend_on_the_block():
    import torch
    from geobipy_amd import gridding, hitmap, pixel_posteriors as pp
    x, y, xe, ye, index, D, dest, src = _geometry("rows")
    rng = np.random.default_rng(8)
    N, nv, nz = x.size, 37, 65
    maps = torch.as_tensor(_maps(rng, N, nv, nz)).cuda()
    lmp = rng.uniform(-4.0, -3.0, N)
    hw, classes, edges = 1.5, ([-2.5, -1.5, -0.5], [0.3, 0.4, 0.5]), np.cumsum(np.concatenate([[0.0], rng.uniform(1.0, 3.0, nz)]))
    plan = gridding.SibsonPlan(x, y, xe, ye, max_distance=6.0 * DX * DY)
    pixels = np.concatenate([np.arange(index.size)[::-1], [4, 4]])
    kw = dict(percentiles=(5, 50, 95), credible=90.0, depth_edges=edges)
    a = pp.products(plan, maps, lmp, hw, pixels=pixels, block=5, classes=classes, **kw)
    b = pp.products(plan, maps, lmp, hw, pixels=pixels, block=10000, classes=classes, **kw)
    part = plan.pool(maps, pixels=pixels, log_mean_prior=lmp, half_width=hw)
    want = hitmap.products(part["pooled"], part["log_mean_prior"], hw, **kw)
    c = hitmap.class_probability(part["pooled"], part["log_mean_prior"], hw, *classes)
    want.update(class_probability=c["probability"], highest_marginal=c["highest_marginal"],
                probability_of_highest_marginal=c["probability_of_highest_marginal"])
    want["clipped_share"] = part["clipped"].double() / (want["total"] + part["clipped"]).double()
    want["count"], want["log_mean_prior"] = part["count"], part["log_mean_prior"]
    assert set(a) == set(b) == set(want) and {"highest_marginal", "clipped_share", "entropy", "percentile_95", "mode"} <= set(a)
    for k in sorted(want):
        _same(a[k].cpu().numpy(), want[k].cpu().numpy(), k + " block 5")
        _same(b[k].cpu().numpy(), want[k].cpu().numpy(), k + " block 10000")
    share = a["clipped_share"].cpu().numpy()
    assert np.isnan(share).any() and (share[~np.isnan(share)] > 0).any() and a["class_probability"].shape == (pixels.size, 3, nz)
    everything = pp.products(plan, maps, lmp, hw, block=7, **kw)               # pixels=None: every pixel, row-major
    _same(everything["median"].cpu().numpy()[pixels], a["median"].cpu().numpy(), "every pixel")
    assert "highest_marginal" not in everything


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


def test_pooled_survey_volume_end_to_end(tmp_path):
    import torch
    from geobipy_amd import gridding, hitmap, survey_volume as sv
    files = _two_lines(tmp_path)
    names = ("median", "percentile_95", "clipped_share")
    dx, dy = 6.0, 4.0
    out = tmp_path / "volume"
    vol = sv.from_lines(str(tmp_path), dx, dy, pooled=True, variables=names, block=50, out=str(out))

    # the composition by hand: plan -> pool -> products
    lines = [sv.load_maps(f) for f in files]
    x, y = np.concatenate([ln[0] for ln in lines]), np.concatenate([ln[1] for ln in lines])
    lmp, hw, d_edges = np.concatenate([ln[4] for ln in lines]), lines[0][5], lines[0][6]
    maps = torch.as_tensor(np.concatenate([ln[3] for ln in lines])).cuda()
    xe, ye = gridding.centred_mesh(x, y, dx, dy)
    plan = gridding.SibsonPlan(x, y, xe, ye)
    ny, nx, nz = plan.ny, plan.nx, maps.shape[2]
    part = plan.pool(maps, log_mean_prior=lmp, half_width=hw)
    assert len({float(v) for v in lmp}) > 2 and part["pooled"].any()          # the lines' soundings have axes of their own
    r = hitmap.products(part["pooled"], part["log_mean_prior"], hw, percentiles=(95.0,), credible=90.0, depth_edges=d_edges)
    r["clipped_share"] = part["clipped"].double() / (r["total"] + part["clipped"]).double()
    _same(vol["x_edges"], xe, "x edges")
    _same(vol["depth_edges"], d_edges, "depth edges")
    assert bool(vol["pooled"]) and bool(np.load(str(out / sv.AXES_FILE))["pooled"])
    for k in names:
        want = r[k].cpu().numpy().T.reshape(nz, ny, nx)
        _same(vol[k], want, k)
        on_file = np.load(sv.pooled_volume_path(str(out), k), mmap_mode="r")
        assert on_file.shape == (nz, ny, nx)
        _same(on_file, want, k + " on file")
        assert not os.path.exists(sv.volume_path(str(out), k))
    assert np.isfinite(vol["median"]).all()

    some = sv.from_lines(list(files), dx, dy, pooled=True, variables=("median", "entropy"), depth=(20, 29), block=1000)
    _same(some["median"], vol["median"][20:30], "cells 20 .. 29")
    _same(some["depth_edges"], d_edges[20:31], "their edges")
    whole = sv.from_lines(list(files), dx, dy, pooled=True, variables=("entropy",), block=7)
    _same(some["entropy"], whole["entropy"][20:30], "the entropy of the whole column, whatever the block")
    one = sv.from_lines(list(files), dx, dy, pooled=True, variables=("median",), depth=7)
    _same(one["median"], vol["median"][7], "depth cell 7")
    with pytest.raises(ValueError, match="banded"):
        sv.from_lines(list(files), dx, dy, pooled=True, variables=("median",), list_budget_bytes=4 * int(plan.count.sum(dim=1).max()))
    with pytest.raises(ValueError, match="interface_probability"):
        sv.from_lines(list(files), dx, dy, pooled=True, variables=("median", "interface_probability"))

    # the command line writes the same arrays
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = tmp_path / "cli"
    p = subprocess.run([sys.executable, "-m", "geobipy_amd.survey_volume", str(tmp_path), "--dx", "6", "--dy", "4", "--pooled", "--variables",
                        *names, "--block", "64", "--out", str(cli)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    assert bool(np.load(str(cli / sv.AXES_FILE))["pooled"])
    for k in names:
        _same(np.load(sv.pooled_volume_path(str(cli), k)), np.asarray(vol[k]), k + " from the command line")
