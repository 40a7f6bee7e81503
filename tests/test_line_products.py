"""Posterior line products (geobipy_amd/line_products.py, csrc/gbp_hitmap.h k_hitmap_products): (i) the torch formulation of the kernel's
column moments (tests/line_products_reference.py) with the package's finishing functions against the imported REFERENCE's own mode,
percentiles, credible range, entropy, opacity, interface pdf and the line's opacity and DOI walk (tests/golden/make_line_products.py ->
line_products.npz) -- CPU tier; the command line's arguments and the C ABI's refusals without a device; (ii) on the GPU the kernel
against the fixture, against the torch formulation on shapes the fixture does not hold (bit for bit on the integer outputs, 1e-13 on
sum c ln c), its mean against ``hitmap.statistics`` bit for bit, and ``from_results`` / the command line end to end on a committed
line container."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import line_products_reference

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "line_products.npz")
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")


def _fixture():
    import torch
    d = dict(np.load(GOLDEN))
    W = float(d["x_edges"][-1])
    nv = d["x_edges"].size - 1
    assert np.allclose(np.diff(d["x_edges"]), 2.0 * W / nv, rtol=0, atol=1e-12) and abs(d["x_edges"][0] + W) < 1e-12
    counts = torch.as_tensor(d["counts"])
    lmp = torch.full((counts.shape[0],), float(d["relative_to"]) * np.log(10.0), dtype=torch.float64)
    return d, counts, lmp, W


def _finish(m, d, lmp, W, nv):
    """The package's finishing functions on the moments: the per-sounding products the fixture records, and the line's."""
    import torch
    from geobipy_amd import hitmap, line_products as lp
    q, pos, (klo, khi) = lp.quantiles(tuple(d["percentiles"]), float(d["credible"]))
    shift = lp.log10_shift(lmp)[:, None]
    centre = lambda i: lp.value_centres(i.cpu(), nv, W, shift).numpy()       # noqa: E731
    out = dict(mode=centre(m["mode_idx"]),
               percentiles=np.stack([centre(m["q_idx"][pos[float(p)]]) for p in d["percentiles"]], axis=1))
    out["credible_range"] = np.abs(centre(m["q_idx"][khi]) - centre(m["q_idx"][klo]))
    area = np.abs(np.diff(d["y_edges"])) * (2.0 * W / nv)
    out["entropy"] = lp.entropy_bits(m["total"].cpu(), m["s1"].cpu(), area).numpy()
    out["opacity"] = np.stack([lp.opacity(r[None])[0].numpy() for r in out["credible_range"]])   # the reference's, one sounding at a time
    out["line_opacity"] = lp.opacity(out["credible_range"]).numpy()
    out["doi_index"] = lp.doi_index(out["line_opacity"], float(d["doi_percent"])).numpy()
    return q, out


def _hold_to_reference(out, d, W, nv):
    cell = 2.0 * W / nv
    assert np.abs(out["mode"] - d["ref_mode"]).max() < 1e-9 * cell, np.abs(out["mode"] - d["ref_mode"]).max() / cell
    assert np.abs(out["percentiles"] - d["ref_percentiles"]).max() < 1e-9 * cell
    for k in ("credible_range", "entropy", "opacity"):
        assert np.abs(out[k] - d["ref_" + k]).max() < 1e-12, (k, np.abs(out[k] - d["ref_" + k]).max())
    assert np.abs(out["line_opacity"] - d["ref_line_opacity"]).max() < 1e-12
    assert np.array_equal(out["doi_index"], d["ref_doi_index"]), (out["doi_index"], d["ref_doi_index"])


def test_torch_moments_and_finishing_equal_the_reference_histogram():
    d, counts, lmp, W = _fixture()
    from geobipy_amd import line_products as lp
    q, _, _ = lp.quantiles(tuple(d["percentiles"]), float(d["credible"]))
    m = line_products_reference.moments_torch(counts, lmp, W, q)
    _, out = _finish(m, d, lmp, W, counts.shape[1])
    _hold_to_reference(out, d, W, counts.shape[1])


def test_interface_pdf_and_doi_walk_equal_the_reference():
    from geobipy_amd import line_products as lp
    d = dict(np.load(GOLDEN))
    line = lp.interface_pdf(d["interface_counts"], d["line_x_edges"], d["y_edges"]).numpy()
    assert np.abs(line - d["ref_line_interface_pdf"]).max() < 1e-12 * max(1.0, np.abs(d["ref_line_interface_pdf"]).max())
    for b in range(d["interface_counts"].shape[0]):                 # one sounding: the 1-D pdf over its depth mesh
        one = lp.interface_pdf(d["interface_counts"][b:b + 1], [-0.5, 0.5], d["y_edges"]).numpy()[0]
        assert np.abs(one - d["ref_interface_pdf"][b]).max() < 1e-15, b
    j = lp.doi_index(d["ref_line_opacity"], float(d["doi_percent"])).numpy()
    assert np.array_equal(j, d["ref_doi_index"])
    # the walk itself: the deepest cell at or above the level, else cell 0, and a NaN stops it as the reference's loop
    op = np.array([[0.9, 0.1, 0.7, 0.2], [0.1, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.67], [0.1, np.nan, 0.1, 0.1]])
    assert lp.doi_index(op, 67.0).tolist() == [2, 0, 3, 1]


def test_transparency_and_entropy_edge_cases():
    import torch
    from geobipy_amd import line_products as lp
    r = np.array([[1.0, np.nan, 3.0], [2.0, 2.0, 1.0]])
    t = lp.transparency(r).numpy()
    assert np.allclose(t, [[0.0, 1.0, 1.0], [0.5, 0.5, 0.0]])
    assert np.array_equal(lp.transparency(np.full((2, 2), 0.4)).numpy(), np.zeros((2, 2)))       # equal extremes: shifted only
    # entropy of a sounding that never counted is 0; of one uniform column over n cells of unit area: log2 n
    tot = torch.tensor([[0, 0], [8, 0]], dtype=torch.int64)
    s1 = torch.tensor([[0.0, 0.0], [4 * 2 * np.log(2.0), 0.0]])     # four cells of 2 counts
    H = lp.entropy_bits(tot, s1, torch.tensor([1.0, 1.0])).numpy()
    assert H[0].tolist() == [0.0, 0.0] and abs(H[1, 0] - 2.0) < 1e-15 and H[1, 1] == 0.0


def test_command_line_arguments(tmp_path):
    from geobipy_amd import line_products as lp
    a = lp.parse_args(["x.h5"])
    assert a.paths == ["x.h5"] and a.credible == 90.0 and a.doi == 67.0 and a.percentiles == [5.0, 50.0, 95.0] and a.block == 4096
    a = lp.parse_args(["a.h5", "d", "--credible", "68", "--doi", "50", "--percentiles", "10", "90"])
    assert a.paths == ["a.h5", "d"] and a.credible == 68.0 and a.doi == 50.0 and a.percentiles == [10.0, 90.0]
    for bad in (["x.h5", "--credible", "100"], ["x.h5", "--doi", "0"], ["x.h5", "--percentiles", "5", "101"],
                ["x.h5", "--percentiles", "1", "2", "3", "4", "6", "7", "8"], ["x.h5", "--block", "0"], []):
        with pytest.raises(SystemExit):
            lp.parse_args(bad)
    for name in ("l1.h5", "l2.hdf5", "l3.results.npz", "notes.txt", "l1.products.npz"):
        (tmp_path / name).write_bytes(b"")
    assert [os.path.basename(f) for f in lp.containers(str(tmp_path))] == ["l1.h5", "l2.hdf5", "l3.results.npz"]
    assert lp.output_path("/d/line_7.h5") == "/d/line_7.products.npz"
    assert lp.output_path("/d/line_7.results.npz") == "/d/line_7.products.npz"
    with pytest.raises(FileNotFoundError):
        lp.containers(str(tmp_path / "missing.h5"))


def test_products_refuse_host_tensors_and_bad_quantiles():
    import torch
    from geobipy_amd import _lib, hitmap
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.products(torch.zeros((1, 4, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.float64), 1.0)
    from geobipy_amd import line_products as lp
    with pytest.raises(ValueError):
        lp.quantiles((5, 50, 95), credible=100.0)
    with pytest.raises(ValueError):
        lp.quantiles((1, 2, 3, 4, 6, 7, 8), credible=90.0)
    q, pos, bounds = lp.quantiles((95, 5), credible=90.0)
    # percentiles: p / 100, the quantiles of hitmap.statistics; the credible bounds: the reference's r_[5, 95] * 0.01
    assert q == [0.05, 0.5, 0.95, 0.9500000000000001] and pos == {5.0: 0, 50.0: 1, 95.0: 2} and bounds == (0, 3)
    assert lp.quantiles((10, 50, 90), credible=80.0)[1:] == ({10.0: 0, 50.0: 1, 90.0: 2}, (0, 2))


def _lib_or_skip():
    from geobipy_amd import _lib
    try:
        return _lib, _lib.load()
    except (_lib.NativeLibraryError, OSError) as e:
        pytest.skip("native library not loadable here: %s" % e)


def test_c_abi_refuses_bad_arguments():
    _lib, lib = _lib_or_skip()
    INVALID = -1
    d = (ctypes.c_double * 8)(0.05, 0.5, 0.95)
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda B, nv, nz, hm, nq, q, ptrs=(p,) * 5: lib.gbp_hitmap_products(B, nv, nz, hm, p, 1.0, nq, q, *ptrs, None)   # noqa: E731
    assert call(0, 250, 440, None, 3, d, (None,) * 5) == 0                       # an empty block: no launch
    assert call(-1, 250, 440, p, 3, d) == INVALID
    assert call(1, 0, 440, p, 3, d) == INVALID
    assert call(1, 250, 0, p, 3, d) == INVALID
    assert call(1, 250, 440, None, 3, d) == INVALID
    assert call(1, 250, 440, p, 9, d) == INVALID
    assert call(1, 250, 440, p, -1, d) == INVALID
    assert call(1, 250, 440, p, 3, None) == INVALID
    assert call(1, 250, 440, p, 3, d, (p, None, p, p, p)) == INVALID
    assert call(1, 250, 440, p, 3, d, (p, p, p, p, None)) == INVALID
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert call(0, 250, 440, None, 1, (ctypes.c_double * 1)(bad), (None,) * 5) == INVALID, bad
    assert b"gbp_hitmap_products" in lib.gbp_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_kernel_equals_the_reference_histogram():
    import torch
    from geobipy_amd import hitmap, line_products as lp
    d, counts, lmp, W = _fixture()
    dev = torch.device("cuda", 0)
    q, _, _ = lp.quantiles(tuple(d["percentiles"]), float(d["credible"]))
    m = hitmap.moments(counts.to(dev), lmp.to(dev), W, q)
    _, out = _finish(m, d, lmp, W, counts.shape[1])
    _hold_to_reference(out, d, W, counts.shape[1])
    # and products() itself: the per-sounding products in the fixture's terms
    p = hitmap.products(counts.to(dev), lmp.to(dev), W, percentiles=tuple(d["percentiles"]), credible=float(d["credible"]),
                        depth_edges=d["y_edges"])
    assert np.abs(p["mode"].cpu().numpy() - d["ref_mode"]).max() < 1e-12
    assert np.abs(p["credible_range"].cpu().numpy() - d["ref_credible_range"]).max() < 1e-12
    assert np.abs(p["entropy"].cpu().numpy() - d["ref_entropy"]).max() < 1e-12
    for k, pc in enumerate(d["percentiles"]):
        assert np.abs(p["percentile_%g" % pc].cpu().numpy() - d["ref_percentiles"][:, k]).max() < 1e-12


def _maps(rng, B, nv, nz):
    hm = np.zeros((B, nv, nz), dtype=np.int32)
    for b in range(B):
        kind = b % 6
        if kind == 0:                                                      # layered posteriors
            for _ in range(40):
                v, (lo, hi) = rng.integers(0, nv), np.sort(rng.integers(0, nz, 2))
                hm[b, v, lo:hi + 1] += rng.integers(1, 900)
        elif kind == 1:                                                    # dense random
            hm[b] = rng.integers(0, 50, (nv, nz))
        elif kind == 2:                                                    # ties everywhere: constant columns
            hm[b] = 3
        elif kind == 3:                                                    # large counts: sum c ln c ~ 1e12
            hm[b] = rng.integers(1 << 22, 1 << 23, (nv, nz)) * (rng.random((nv, nz)) < 0.5)
        elif kind == 4:                                                    # cumulative shares on the quantiles: 1, 9, 9, 1 of 20
            if nv >= 4:
                for z in range(nz):
                    hm[b, np.sort(rng.choice(nv, 4, replace=False)), z] = (1, 9, 9, 1)
            else:
                hm[b, 0] = 1
        # kind 5: empty
    return hm


@pytest.mark.gpu
def test_kernel_equals_the_torch_formulation():
    import torch
    from geobipy_amd import hitmap
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    qsets = ([0.05, 0.5, 0.9500000000000001], [0.01, 0.16, 0.25, 0.5, 0.75, 0.84, 0.99, 0.999], [0.5], [])
    n = 0
    for B in (0, 1, 37):
        for nv in (1, 250, 257):
            for nz in (1, 255, 257, 440):
                if B == 37 and nv > 1 and nz in (1, 255):
                    continue                                                # (enough of the big ones)
                hm = torch.as_tensor(_maps(rng, B, nv, nz), device=dev)
                lmp = torch.as_tensor(rng.normal(-4.0, 0.5, B), device=dev)
                q = qsets[n % len(qsets)]
                n += 1
                m = hitmap.moments(hm, lmp, 2.3, q)
                r = line_products_reference.moments_torch(hm, lmp, 2.3, q)
                tag = (B, nv, nz, len(q))
                assert torch.equal(m["total"], r["total"]), tag
                assert torch.equal(m["mode_idx"], r["mode_idx"]), tag
                assert torch.equal(m["q_idx"], r["q_idx"]), tag
                rel = ((m["s1"] - r["s1"]).abs() / r["s1"].abs().clamp(min=1e-300)).max() if B else torch.zeros(())
                assert float(rel) <= 1e-13, (tag, float(rel))
                assert torch.allclose(m["mean"], r["mean"], rtol=0, atol=1e-12), tag
                if B:
                    mean, _ = hitmap.statistics(hm, lmp, 2.3)
                    assert torch.equal(m["mean"], mean), tag                # the bits of gbp_hitmap_statistics
    assert n > 20


@pytest.mark.gpu
def test_products_percentiles_have_the_bits_of_statistics():
    import torch
    from geobipy_amd import hitmap
    dev = torch.device("cuda", 0)
    hm = torch.as_tensor(_maps(np.random.default_rng(8), 12, 250, 440), device=dev)
    lmp = torch.as_tensor(np.random.default_rng(9).normal(-4.0, 0.5, 12), device=dev)
    p = hitmap.products(hm, lmp, 2.3)
    mean, pct = hitmap.statistics(hm, lmp, 2.3)
    assert torch.equal(p["mean"], mean) and torch.equal(p["percentile_50"], pct[1]) and torch.equal(p["median"], pct[1])
    assert torch.equal(p["percentile_5"], pct[0]) and torch.equal(p["percentile_95"], pct[2])


def _expected_from_arrays(path, percentiles=(5, 50, 95), credible=90.0, doi=67.0):
    """The torch formulation plus the host arithmetic on the container's own arrays."""
    import torch
    from geobipy_amd import hdf, line_products as lp
    a, _ = hdf.load_results(path)
    hm = torch.as_tensor(a[lp.VALUES + "/values/data"])
    e = a[lp.VALUES + "/mesh/y/edges/data"]
    de = a[lp.VALUES + "/mesh/z/edges/data"]
    W, nv = float(e[-1]), hm.shape[1]
    lmp = torch.as_tensor(np.asarray(a[lp.VALUES + "/mesh/y/relative_to/data"], dtype=np.float64) * lp.LN10)
    q, pos, (klo, khi) = lp.quantiles(percentiles, credible)
    m = line_products_reference.moments_torch(hm, lmp, W, q)
    shift = lp.log10_shift(lmp)[:, None]
    c = lambda i: lp.value_centres(i, nv, W, shift).numpy()                 # noqa: E731
    out = dict(median=c(m["q_idx"][pos[50.0]]), mode=c(m["mode_idx"]), credible_range=np.abs(c(m["q_idx"][khi]) - c(m["q_idx"][klo])))
    for p in percentiles:
        out["percentile_%g" % p] = c(m["q_idx"][pos[float(p)]])
    out["entropy"] = lp.entropy_bits(m["total"], m["s1"], np.abs(np.diff(de)) * (2.0 * W / nv)).numpy()
    out["opacity"] = lp.opacity(out["credible_range"]).numpy()
    out["doi_index"] = lp.doi_index(out["opacity"], doi).numpy()
    out["doi_depth"] = (0.5 * (de[1:] + de[:-1]))[out["doi_index"]]
    out["doi_elevation"] = np.asarray(a["/data/elevation/data"]) - out["doi_depth"]
    out["interface_probability"] = lp.interface_pdf(a[lp.INTERFACES + "/values/data"], a[lp.INTERFACES + "/mesh/x/edges/data"],
                                                    a[lp.INTERFACES + "/mesh/y/edges/data"]).numpy()
    out["mean"] = m["mean"].numpy()
    return out


def _check_products(got, want):
    for k in ("median", "mode", "percentile_5", "percentile_50", "percentile_95", "doi_index", "doi_depth", "doi_elevation"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("credible_range", "entropy", "opacity", "interface_probability", "mean"):
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k


@pytest.mark.gpu
def test_from_results_end_to_end():
    from geobipy_amd import line_products as lp
    got = lp.from_results(SURVEY, block=3)                                   # three uploads of a line of eight
    want = _expected_from_arrays(SURVEY)
    assert got["mean"].shape == (8, 440) and got["opacity"].min() >= 0.0 and got["opacity"].max() <= 1.0
    _check_products(got, want)
    assert np.array_equal(lp.from_results(SURVEY)["opacity"], got["opacity"])   # (the block size changes nothing)


@pytest.mark.gpu
def test_command_line_writes_products(tmp_path):
    import shutil
    src = str(tmp_path / "line_0.h5")
    shutil.copy(SURVEY, src)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.line_products", str(tmp_path), "--percentiles", "10", "50", "90"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "line_0.products.npz"
    assert out.exists(), r.stdout
    got = dict(np.load(str(out)))
    want = _expected_from_arrays(SURVEY, percentiles=(10, 50, 90))
    for k in ("percentile_10", "percentile_90", "median", "doi_depth"):
        assert np.array_equal(got[k], want[k]), k
    assert float(got["credible"]) == 90.0 and float(got["doi_percent"]) == 67.0
