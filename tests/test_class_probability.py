"""Class (lithology) probabilities of the hit maps (csrc/gbp_hitmap.h k_hitmap_classes, geobipy_amd/hitmap.py class_probability,
line_products.from_results(classes=...)): (i) the torch formulation (tests/class_probability_reference.py) against the imported
REFERENCE's own ``compute_probability(..., log=10, axis=0)`` and its argmax over the class axis (tests/golden/make_class_probability.py ->
class_probability.npz), the command line's class arguments and the C ABI's refusals -- CPU tier; (ii) on the GPU the kernel against the
fixture and against the torch formulation on many shapes, and ``from_results`` / the command line end to end on a committed line
container.

Probabilities are compared at rtol 1e-10 with an absolute floor of 1e-250: a class whose sum holds only terms near or below the
subnormal range (a Gaussian weight e^-700 of a narrow class) carries the rounding of a subnormal ulp, relative to the column's total;
the recorder keeps the LARGEST term of every column normal, so that every probability above the floor is held to rtol."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import class_probability_reference

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "class_probability.npz")
MAPS = os.path.join(HERE, "golden", "line_products.npz")
SURVEY = os.path.join(HERE, "golden", "device_survey_0.0.h5")
RTOL, ATOL = 1e-10, 1e-250
CLASSES = ([-2.5, -1.5, -0.5], [0.3, 0.3, 0.4])


def _fixture():
    import torch
    d = dict(np.load(GOLDEN))
    m = dict(np.load(MAPS))
    W = float(m["x_edges"][-1])
    counts = torch.as_tensor(m["counts"])
    lmp = torch.full((counts.shape[0],), float(m["relative_to"]) * np.log(10.0), dtype=torch.float64)
    return d, counts, lmp, W


def _same_probabilities(got, want, tag=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str(tag))


def _hold_to_fixture(out, d, name):
    _same_probabilities(out["probability"], d["prob_" + name], name)
    assert np.array_equal(np.asarray(out["highest_marginal"]), d["best_" + name]), name
    _same_probabilities(out["probability_of_highest_marginal"], d["best_p_" + name], name)


def test_torch_formulation_equals_the_reference():
    d, counts, lmp, W = _fixture()
    assert sorted(d["sets"]) == ["a", "b", "c", "d", "e"]
    for name in d["sets"]:
        out = class_probability_reference.class_probability_torch(counts, lmp, W, d["means_" + name], d["scales_" + name])
        _hold_to_fixture({k: v.numpy() for k, v in out.items()}, d, name)
    # what the sets hold: empty columns (and an empty map) are NaN; set e underflows everywhere; set c's twin classes tie, the first wins
    assert np.isnan(d["prob_a"][7]).all() and np.isnan(d["prob_e"]).all() and (d["best_e"] == 0).all()
    twin = ~np.isnan(d["best_p_c"]) & (d["prob_c"][:, 2] == d["best_p_c"])
    assert twin.any() and (d["best_c"][twin] == 2).all() and np.array_equal(d["prob_c"][:, 2], d["prob_c"][:, 5], equal_nan=True)
    fin = ~np.isnan(d["prob_b"][:, 0])
    assert np.abs(d["prob_b"].sum(axis=1)[fin] - 1.0).max() < 1e-12


def test_command_line_class_arguments():
    from geobipy_amd import line_products as lp
    a = lp.parse_args(["x.h5"])
    assert a.class_means is None and a.class_scales is None
    a = lp.parse_args(["x.h5", "--class-means", "-2.5", "-1.5", "-0.5", "--class-scales", "0.3", "0.3", "0.4"])
    assert a.class_means == [-2.5, -1.5, -0.5] and a.class_scales == [0.3, 0.3, 0.4]
    a = lp.parse_args(["x.h5", "--class-means"] + ["%d" % i for i in range(16)] + ["--class-scales"] + ["1"] * 16)
    assert len(a.class_means) == 16
    for bad in (["x.h5", "--class-means", "-1"], ["x.h5", "--class-scales", "0.3"],
                ["x.h5", "--class-means", "-1", "-2", "--class-scales", "0.3"],
                ["x.h5", "--class-means"] + ["0"] * 17 + ["--class-scales"] + ["1"] * 17,
                ["x.h5", "--class-means", "-1", "--class-scales", "0"], ["x.h5", "--class-means", "-1", "--class-scales", "-0.3"],
                ["x.h5", "--class-means", "-1", "--class-scales", "nan"], ["x.h5", "--class-means", "inf", "--class-scales", "1"]):
        with pytest.raises(SystemExit):
            lp.parse_args(bad)
    with pytest.raises(ValueError):
        lp.from_results(SURVEY, classes=([-1.0, 0.0], [0.5]))


def test_class_probability_refuses_host_tensors():
    import torch
    from geobipy_amd import _lib, hitmap
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.class_probability(torch.zeros((1, 4, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.float64), 1.0, [0.0], [1.0])


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
    D = lambda *x: (ctypes.c_double * len(x))(*x)          # noqa: E731
    mu, sd = D(-2.0, -1.0, 0.0), D(0.3, 0.3, 0.4)

    def call(B=1, nv=250, nz=440, hm=p, lmp=p, K=3, means=mu, scales=sd, outs=(p, p, p)):
        return lib.gbp_hitmap_classes(B, nv, nz, hm, lmp, 1.0, K, means, scales, *outs, None)

    assert call(B=0, hm=None, lmp=None, outs=(None,) * 3) == 0                   # an empty block: no launch
    assert call(B=0, nv=1024, K=8, means=D(*range(8)), scales=D(*[1.0] * 8), hm=None, lmp=None, outs=(None,) * 3) == 0   # 64 KiB: fits
    assert call(B=-1) == INVALID
    assert call(nv=0) == INVALID and call(nv=-3) == INVALID
    assert call(nz=0) == INVALID and call(nz=-1) == INVALID
    assert call(K=0) == INVALID and call(K=-1) == INVALID
    assert call(K=17, means=D(*range(17)), scales=D(*[1.0] * 17)) == INVALID
    for bad in (0.0, -0.3, float("inf"), float("nan")):
        assert call(scales=D(0.3, bad, 0.4)) == INVALID, bad
        assert call(B=0, scales=D(0.3, bad, 0.4), hm=None, lmp=None, outs=(None,) * 3) == INVALID, bad     # (checked before B == 0)
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert call(means=D(bad, 0.0, 1.0)) == INVALID, bad
    assert call(B=0, nv=1025, K=8, means=D(*range(8)), scales=D(*[1.0] * 8), hm=None, lmp=None, outs=(None,) * 3) == INVALID   # LDS
    assert call(nv=513, K=16, means=D(*range(16)), scales=D(*[1.0] * 16)) == INVALID
    assert call(means=None) == INVALID and call(scales=None) == INVALID
    assert call(hm=None) == INVALID and call(lmp=None) == INVALID
    for i in range(3):
        outs = [p, p, p]
        outs[i] = None
        assert call(outs=tuple(outs)) == INVALID, i
    assert call(B=1 << 20, nz=1 << 12, nv=1) == INVALID                          # B * n_depth beyond int32
    assert b"gbp_hitmap_classes" in lib.gbp_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_kernel_equals_the_reference():
    import torch
    from geobipy_amd import hitmap
    d, counts, lmp, W = _fixture()
    dev = torch.device("cuda", 0)
    for name in d["sets"]:
        out = hitmap.class_probability(counts.to(dev), lmp.to(dev), W, d["means_" + name], d["scales_" + name])
        assert out["highest_marginal"].dtype == torch.int32
        _hold_to_fixture({k: v.cpu().numpy() for k, v in out.items()}, d, name)


def _maps(rng, B, nv, nz):
    hm = np.zeros((B, nv, nz), dtype=np.int32)
    big = (1 << 31) // nv                                                      # a column of these sums to just under 2^31
    for b in range(B):
        kind = b % 5
        if kind == 0:                                                          # layered posteriors
            for _ in range(40):
                v, (lo, hi) = rng.integers(0, nv), np.sort(rng.integers(0, nz, 2))
                hm[b, v, lo:hi + 1] += rng.integers(1, 900)
        elif kind == 1:                                                        # dense random
            hm[b] = rng.integers(0, 50, (nv, nz))
        elif kind == 2:                                                        # constant columns
            hm[b] = 3
        elif kind == 3:                                                        # counts near 2^31 / nv
            hm[b] = rng.integers(big - big // 8, big, (nv, nz))
        # kind 4: empty
    return hm


def _classes(rng, K, lo, hi):
    means = rng.uniform(lo, hi, K)
    scales = rng.uniform(0.05, 1.0, K)
    return means, scales


def _check_against_torch(hm, lmp, W, means, scales, tag):
    from geobipy_amd import hitmap
    got = hitmap.class_probability(hm, lmp, W, means, scales)
    want = class_probability_reference.class_probability_torch(hm, lmp, W, means, scales)
    P, R = got["probability"].cpu().numpy(), want["probability"].cpu().numpy()
    _same_probabilities(P, R, tag)
    _same_probabilities(got["probability_of_highest_marginal"].cpu().numpy(), want["probability_of_highest_marginal"].cpu().numpy(), tag)
    j, jr = got["highest_marginal"].cpu().numpy(), want["highest_marginal"].cpu().numpy()
    off = j != jr                                          # (only where two classes agree to rounding: the kernel's pick is a maximum too)
    if off.any():
        pick = np.take_along_axis(R, j[:, None].astype(np.int64), axis=1)[:, 0]
        top = np.where(np.isnan(R), -np.inf, R).max(axis=1)
        assert np.all(np.abs(pick[off] - top[off]) <= RTOL * np.abs(pick[off])), tag
    fin = ~np.isnan(P[:, 0])
    if fin.any():
        assert np.abs(P.sum(axis=1)[fin] - 1.0).max() < 1e-12, tag
    return P


@pytest.mark.gpu
def test_kernel_equals_the_torch_formulation():
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    Ks = (1, 2, 5, 8, 16)
    n = 0
    for B in (1, 3, 257):
        for nv in (1, 7, 250, 1000):
            for nz in (1, 255, 256, 257, 440):
                if B == 257 and (nv, nz) not in ((1, 257), (7, 440), (7, 1), (250, 256)):
                    continue                                                   # (enough of the big ones)
                K = Ks[n % len(Ks)]
                while K * nv > 8192:
                    K //= 2
                hm = torch.as_tensor(_maps(rng, B, nv, nz), device=dev)
                lmp = torch.as_tensor(rng.normal(-4.0, 0.5, B), device=dev)
                W = 2.3
                means, scales = _classes(rng, K, -4.0 - W - 0.5, -4.0 + W + 0.5)
                _check_against_torch(hm, lmp, W, means, scales, (B, nv, nz, K))
                n += 1
    assert n > 40


@pytest.mark.gpu
def test_kernel_lds_limit_empty_maps_and_underflow():
    import torch
    from geobipy_amd import _lib, hitmap
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    for K, nv in ((8, 1024), (16, 512), (1, 8192), (5, 1638)):               # K n_value 8 B = 64 KiB exactly, or just under it
        hm = torch.as_tensor(_maps(rng, 5, nv, 257), device=dev)
        lmp = torch.as_tensor(rng.normal(-2.0, 0.3, 5), device=dev)
        P = _check_against_torch(hm, lmp, 3.0, *_classes(rng, K, -5.0, 1.0), (K, nv))
        assert np.isnan(P[4]).all() and not np.isnan(P[0:4, :, :]).all()       # sounding 4: an empty map
    for K, nv in ((8, 1025), (16, 513), (2, 4097)):
        hm = torch.zeros((2, nv, 3), dtype=torch.int32, device=dev)
        with pytest.raises(_lib.NativeLibraryError, match="LDS"):
            hitmap.class_probability(hm, torch.zeros(2, dtype=torch.float64, device=dev), 1.0, [0.0] * K, [1.0] * K)
    # classes far from every cell: each term is exactly 0 -> NaN, class 0 the "most probable"
    hm = torch.as_tensor(_maps(rng, 4, 250, 440), device=dev)
    out = hitmap.class_probability(hm, torch.full((4,), -4.0, dtype=torch.float64, device=dev), 2.3, [60.0, -80.0], [0.5, 0.3])
    assert torch.isnan(out["probability"]).all() and torch.isnan(out["probability_of_highest_marginal"]).all()
    assert (out["highest_marginal"] == 0).all()
    # an empty block
    out = hitmap.class_probability(torch.zeros((0, 250, 440), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float64, device=dev),
                                   2.3, [0.0, 1.0], [1.0, 1.0])
    assert out["probability"].shape == (0, 2, 440) and out["highest_marginal"].shape == (0, 440)


@pytest.mark.gpu
def test_from_results_with_classes():
    import torch
    from geobipy_amd import hdf, line_products as lp
    plain = lp.from_results(SURVEY, block=3)
    got = lp.from_results(SURVEY, classes=CLASSES, block=3)
    whole = lp.from_results(SURVEY, classes=CLASSES, block=4096)
    new = {"class_probability", "highest_marginal", "probability_of_highest_marginal", "class_means", "class_scales"}
    assert set(got) == set(plain) | new and set(whole) == set(got)
    for k in plain:                                                            # the products are untouched by the classes
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    for k in new:
        assert np.asarray(got[k]).tobytes() == np.asarray(whole[k]).tobytes(), k  # (the block size changes nothing)
    N, nz = plain["mean"].shape
    assert got["class_probability"].shape == (N, 3, nz) and got["highest_marginal"].shape == (N, nz)
    assert got["highest_marginal"].dtype == np.int32
    assert np.array_equal(got["class_means"], CLASSES[0]) and np.array_equal(got["class_scales"], CLASSES[1])
    a, _ = hdf.load_results(SURVEY)
    hm = torch.as_tensor(a[lp.VALUES + "/values/data"])
    W = float(a[lp.VALUES + "/mesh/y/edges/data"][-1])
    lmp = torch.as_tensor(np.asarray(a[lp.VALUES + "/mesh/y/relative_to/data"], dtype=np.float64).reshape(-1) * lp.LN10)
    want = class_probability_reference.class_probability_torch(hm, torch.broadcast_to(lmp, (N,)).contiguous(), W, *CLASSES)
    _same_probabilities(got["class_probability"], want["probability"].numpy())
    fin = ~np.isnan(got["class_probability"][:, 0])
    assert fin.any() and np.abs(got["class_probability"].sum(axis=1)[fin] - 1.0).max() < 1e-12


@pytest.mark.gpu
def test_command_line_writes_class_probability(tmp_path):
    import shutil
    src = str(tmp_path / "line_0.h5")
    shutil.copy(SURVEY, src)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "geobipy_amd.line_products", str(tmp_path), "--class-means", "-2.5", "-1.5", "-0.5",
                        "--class-scales", "0.3", "0.3", "0.4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = dict(np.load(str(tmp_path / "line_0.products.npz")))
    N, nz = got["mean"].shape
    assert got["class_probability"].shape == (N, 3, nz)
    fin = ~np.isnan(got["class_probability"][:, 0])
    assert fin.any() and np.abs(got["class_probability"].sum(axis=1)[fin] - 1.0).max() < 1e-12
    assert got["highest_marginal"].shape == (N, nz) and got["probability_of_highest_marginal"].shape == (N, nz)
    assert np.array_equal(got["class_means"], [-2.5, -1.5, -0.5]) and np.array_equal(got["class_scales"], [0.3, 0.3, 0.4])
