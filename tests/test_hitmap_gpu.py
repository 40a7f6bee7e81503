"""csrc/gbp_hitmap.h: (i) the per-depth statistics against the imported REFERENCE's own ``Histogram.mean`` / ``Histogram.percentile``
on recorded hit maps (tests/golden/make_hitmap_stats.py -> hitmap_stats.npz: layered posteriors, one cell per depth, cumulative shares
that fall exactly on a percentile, empty columns) -- the torch formulation on the CPU tier, the kernel on the GPU tier; (ii) the kernels
against the torch formulations (tests/hitmap_reference.py) on shapes the fixture does not hold: the run-length form of the hit maps bit
for bit (rows of every kind: empty, constant, alternating, a change at every tile border, a length that is no multiple of the tile),
the statistics cell for cell."""
import os

import numpy as np
import pytest

import hitmap_reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hitmap_stats.npz")


def _fixture():
    import torch
    d = np.load(GOLDEN)
    W = float(d["x_edges"][-1])
    assert np.allclose(np.diff(d["x_edges"]), 2.0 * W / (d["x_edges"].size - 1), rtol=0, atol=1e-12) and abs(d["x_edges"][0] + W) < 1e-12
    counts = torch.as_tensor(d["counts"])
    lmp = torch.full((counts.shape[0],), float(d["relative_to"]) * np.log(10.0), dtype=torch.float64)   # the device carries ln, the mesh log10
    # the reference returns S/m (10 ** (value + relative_to)); the kernel log10
    return counts, lmp, W, np.log10(d["ref_mean"]), np.log10(d["ref_percentiles"])


def _hold_to_reference(mean, pct, ref_mean, ref_pct, W, nv):
    cell = 2.0 * W / nv
    assert np.abs(mean - ref_mean).max() < 1e-12, np.abs(mean - ref_mean).max()
    for q in range(3):                                # the SAME cell (its centre to rounding), ties and empty columns included
        assert np.abs(pct[q] - ref_pct[:, q]).max() < 1e-9 * cell, (q, np.abs(pct[q] - ref_pct[:, q]).max() / cell)


def test_torch_formulation_equals_the_reference_histogram():
    counts, lmp, W, ref_mean, ref_pct = _fixture()
    mean, pct = hitmap_reference.statistics_torch(counts, lmp, W)
    _hold_to_reference(mean.numpy(), [p.numpy() for p in pct], ref_mean, ref_pct, W, counts.shape[1])


@pytest.mark.gpu
def test_hitmap_statistics_kernel_equals_the_reference_histogram():
    import torch
    from geobipy_amd import hitmap
    counts, lmp, W, ref_mean, ref_pct = _fixture()
    dev = torch.device("cuda", 0)
    mean, pct = hitmap.statistics(counts.to(dev), lmp.to(dev), W)
    _hold_to_reference(mean.cpu().numpy(), [p.cpu().numpy() for p in pct], ref_mean, ref_pct, W, counts.shape[1])


@pytest.mark.gpu
def test_hitmap_runs_and_statistics_equal_the_torch_formulations():
    import torch
    from geobipy_amd import hitmap
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    for B, nv, nz in ((7, 250, 440), (3, 5, 7), (2, 1, 1), (5, 13, 1024), (4, 4, 257)):
        M = nv * nz
        hm = np.zeros((B, nv, nz), dtype=np.int32)
        for b in range(B):
            kind = b % 7
            if kind == 1:
                hm[b] = 9
            elif kind == 2:
                hm[b].reshape(-1)[::2] = 1
            elif kind == 3:
                hm[b].reshape(-1)[np.arange(0, M, 256)] = rng.integers(1, 5, np.arange(0, M, 256).size)       # changes at the sub-tile borders
                hm[b].reshape(-1)[np.arange(255, M, 1024)] = -3
            elif kind == 4:
                hm[b] = rng.integers(0, 3, (nv, nz)) * (rng.random((nv, nz)) < 0.02)
            elif kind >= 5:
                for _ in range(60):                                        # layered posteriors
                    v, lo, hi = rng.integers(0, nv), *np.sort(rng.integers(0, nz, 2))
                    hm[b, v, lo:hi + 1] += rng.integers(1, 900)
        t = torch.as_tensor(hm, device=dev)
        ptr, start, value = hitmap.runs(t)
        ptr0, start0, value0 = hitmap_reference.runs_torch(t)
        assert torch.equal(ptr, ptr0) and torch.equal(start, start0) and torch.equal(value, value0.to(torch.int32)), (B, nv, nz)
        assert ptr.dtype == torch.int64 and start.dtype == torch.int32
        lmp = torch.as_tensor(rng.normal(-4.0, 0.5, B), device=dev)
        mean, pct = hitmap.statistics(t, lmp, 2.3)
        mean0, pct0 = hitmap_reference.statistics_torch(t, lmp, 2.3)
        assert torch.allclose(mean, mean0, rtol=0, atol=1e-12), float((mean - mean0).abs().max())
        for a_, b_ in zip(pct, pct0):                  # neighbouring cells are 2 * 2.3 / nv apart: the same cell, its centre to rounding
            assert torch.allclose(a_, b_, rtol=0, atol=1e-12), (B, nv, nz, float((a_ - b_).abs().max()))
    # the numpy form the containers take (hdf._Dataset.write_run_rows) expands back to the maps
    from geobipy_amd import hdf
    d = hdf._Dataset("/x", shape=hm.shape, dtype="i4", fillvalue=0)
    d.write_run_rows(np.arange(B), ptr.cpu().numpy(), start.cpu().numpy(), value.cpu().numpy())
    assert np.array_equal(d.arr, hm)


@pytest.mark.gpu
def test_launches_follow_torchs_current_stream():
    """``_lib.call`` launches on torch's current stream of the tensors' device: under ``torch.cuda.stream(side)`` a value-axis
    reduction (hitmap.statistics) and a chain with a back-pointer (sections.track) give the default stream's bits."""
    import torch
    from geobipy_amd import hitmap, sections
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    hm = torch.as_tensor(rng.integers(0, 9, (2, 4, 3)).astype(np.int32), device=dev)
    lmp = torch.as_tensor(rng.normal(-4.0, 0.5, 2), device=dev)
    d2 = torch.as_tensor(rng.uniform(0.0, 2.0, (3, 2, 2)), device=dev)
    g, ptr, n_used = np.array([0.7, 1.3, 1.0]), [0, 3], np.array([2, 2, 2])
    mean0, pct0 = hitmap.statistics(hm, lmp, 2.3)
    track0 = sections.track(d2, g, ptr, n_used)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        mean1, pct1 = hitmap.statistics(hm, lmp, 2.3)
        track1 = sections.track(d2, g, ptr, n_used)
    side.synchronize()
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t      # noqa: E731
    assert torch.equal(bits(mean0), bits(mean1))
    for a, b in zip(pct0, pct1):
        assert torch.equal(bits(a), bits(b))
    assert set(track0) == set(track1) == {"state", "log_score", "marginal", "log_partition", "scale"}
    for name in track0:
        assert torch.equal(bits(track0[name]), bits(track1[name])), name


@pytest.mark.gpu
def test_blocks_of_soundings_pass_the_marshalling_check_with_the_same_bits():
    """families.distance in blocks of two soundings out of three -- the slices k[s], edges[s], sigma[s], rows[s] and out[s], the last
    block shorter -- through ``_lib.call``: the bits of one launch."""
    import torch
    from geobipy_amd import ensembles, families
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    B, ns, K, n = 3, 4, 3, 2
    k = rng.integers(1, K + 1, (B, ns)).astype(np.int32)
    edges = np.sort(rng.uniform(1.0, 90.0, (B, ns, K)), axis=2)
    sigma = 10.0 ** rng.uniform(-3.0, 0.0, (B, ns, K))
    ens = ensembles.Ensemble(*(torch.as_tensor(a).to(dev) for a in (k, edges, sigma)), None, None, 1, None)
    rows = torch.as_tensor(np.array([[0, 3], [2, 1], [1, 1]], dtype=np.int32)).to(dev)
    one = families.distance(ens, rows, 0.0, 100.0, block=None)
    two = families.distance(ens, rows, 0.0, 100.0, block=2)
    assert one.shape == (B, n, n) and bool(torch.isfinite(one).all()) and float(one[0, 0, 1]) > 0.0
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
