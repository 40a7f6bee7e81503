"""Replicate chains (geobipy_amd/replicates.py, hitmap.pool, csrc/gbp_hitmap.h k_hitmap_pool): C chains per sounding,
their posteriors pooled and their agreement mapped per depth cell.  The reference has no counterpart: the rule is stated on the host
(replicates.pool_reference), checked here against its closed forms, and the kernel is held to it."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from geobipy_amd import replicates, survey

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTIONS = os.path.join(GOLDEN, "resolve_options_small")
SHORT = dict(n_markov_chains=1500, burn_in_min_iterations=300, check_every=300)       # a short schedule for the survey runs
CHAIN_KEYS = ("n_markov_chains", "solve_gradient", "maximum_number_of_layers", "minimum_depth", "maximum_depth", "minimum_thickness",
              "initial_relative_error", "minimum_relative_error", "maximum_relative_error", "initial_additive_error", "minimum_additive_error",
              "maximum_additive_error", "relative_error_proposal_variance", "additive_error_proposal_variance", "probability_of_birth",
              "probability_of_death", "probability_of_perturb", "probability_of_no_change", "factor", "gradient_standard_deviation",
              "covariance_scaling", "parameter_limits", "update_plot_every", "reset_limit", "solve_parameter", "solve_relative_error",
              "solve_additive_error")


# -- the host rule: closed forms -----------------------------------------------------------------------------------------------------

def test_identical_chains_give_the_closed_forms():
    rng = np.random.default_rng(1)
    for C in (2, 3, 8):
        one = rng.integers(0, 40, size=(1, 9, 5))
        one[0, 4, :] += 1                                           # (no empty column)
        r = replicates.pool_reference(np.tile(one, (C, 1, 1)), C, None, 1.3)
        n = one[0].sum(axis=0).astype(np.float64)
        assert np.array_equal(r["pooled"], C * one) and np.all(r["n_used"] == C)
        assert np.allclose(r["rhat"][0], np.sqrt((n - 1.0) / n), rtol=1e-12, atol=0.0)         # Bn is exactly 0
        assert np.all(np.abs(r["jsd"][0]) <= 1e-12)
        x = ((np.arange(9) + 0.5) / 9) * 2.6 - 1.3
        assert np.allclose(r["chain_mean"][0, 0], (one[0] * x[:, None]).sum(axis=0) / n, rtol=1e-12)


def test_disjoint_and_coincident_single_bins():
    for C in (2, 4, 5, 8):
        h = np.zeros((C, 8, 2), dtype=np.int64)
        for c in range(C):
            h[c, c, 0] = 16                                         # column 0: every chain in a bin of its own
            h[c, 3, 1] = 16 + c                                     # column 1: every chain in the same bin
        r = replicates.pool_reference(h, C, None, 2.0)
        assert abs(r["jsd"][0, 0] - math.log2(C)) <= 1e-12 and r["rhat"][0, 0] == np.inf
        assert r["rhat"][0, 1] == 1.0 and abs(r["jsd"][0, 1]) <= 1e-12


def test_fewer_than_two_chains_give_nan():
    h = np.zeros((6, 5, 3), dtype=np.int64)
    h[:, 1:4, :] = 7
    h[1:3, :, 1] = 0                                                # sounding 0, column 1: only chain 0 has samples
    use = np.array([[1, 1, 1], [0, 1, 0]])                          # sounding 1: one chain in use
    r = replicates.pool_reference(h, 3, use, 1.0)
    assert np.array_equal(r["n_used"], [[3, 1, 3], [1, 1, 1]])
    assert np.isnan(r["rhat"][0, 1]) and np.isnan(r["jsd"][0, 1]) and np.isfinite(r["rhat"][0, 0]) and np.isfinite(r["jsd"][0, 2])
    assert np.isnan(r["rhat"][1]).all() and np.isnan(r["jsd"][1]).all()
    assert np.array_equal(r["pooled"][1], h[4]) and np.isnan(r["chain_mean"][1, 0]).all() and np.isfinite(r["chain_mean"][1, 1]).all()
    assert np.isnan(r["chain_mean"][0, 1, 1]) and np.isnan(r["chain_mean"][0, 2, 1])


# -- host functions and argument checks ----------------------------------------------------------------------------------------------

def test_expand_keeps_replicate_zero_and_makes_unique_ids():
    rows = np.array([3, 4, 9])
    row, cid = replicates.expand(rows, 3, 10)
    assert row.tolist() == [3, 3, 3, 4, 4, 4, 9, 9, 9] and cid.dtype == np.int64
    assert np.array_equal(cid[0::3], rows)                         # replicate 0: the id the sounding has alone
    assert cid.tolist() == [3, 13, 23, 4, 14, 24, 9, 19, 29]
    _, all_ids = replicates.expand(np.arange(10), 8, 10)
    assert np.unique(all_ids).size == 80
    with pytest.raises(ValueError):
        replicates.expand([10], 2, 10)


def test_pool_refuses_bad_arguments():
    from geobipy_amd import _lib, hitmap
    ok = torch.ones((6, 4, 5), dtype=torch.int32)
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.pool(ok, 3)                                          # a host tensor: no fallback
    with pytest.raises(TypeError):
        hitmap.pool(ok.to(torch.int64), 3)
    with pytest.raises(ValueError):
        hitmap.pool(ok, 4)                                          # 6 maps are not 4 chains per sounding
    with pytest.raises(ValueError):
        hitmap.pool(ok, 1)
    with pytest.raises(ValueError):
        hitmap.pool(ok, 9)
    with pytest.raises(ValueError):
        hitmap.pool(ok.transpose(1, 2), 3)                          # not contiguous
    with pytest.raises(ValueError):
        hitmap.pool(ok, 3, use=torch.ones(6))
    big = torch.zeros((2, 2, 1), dtype=torch.int32)
    big[:, 0, 0] = (1 << 30) - 1
    big[:, 1, 0] = 1
    with pytest.raises(ValueError, match="2\\^31"):
        hitmap.pool(big, 2)                                         # 2 x 2^30 samples in a column: a pooled cell could overflow
    big[:, 1, 0] = 0
    with pytest.raises(_lib.NativeLibraryError):
        hitmap.pool(big, 2)                                         # 2 x (2^30 - 1) fits: only the device is missing


def test_c_abi_refuses_bad_arguments():
    from geobipy_amd import _lib
    lib = _lib.load()                                               # (a library that does not load is a failure, not a skip)
    assert "gbp_hitmap_pool" in _lib.SIGNATURES
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(S=1, C=4, nv=250, nz=440, hm=p, use=p, pooled=p, n_used=p, cm=p, rhat=p, jsd=p):
        return lib.gbp_hitmap_pool(S, C, nv, nz, hm, use, 1.0, pooled, n_used, cm, rhat, jsd, None)

    none = dict(hm=None, use=None, pooled=None, n_used=None, cm=None, rhat=None, jsd=None)
    assert call(S=0, **none) == 0                                   # an empty block: no launch
    assert call(S=0, C=1, **none) == INVALID and call(S=0, C=9, **none) == INVALID       # (checked before S == 0)
    assert call(C=1) == INVALID and call(C=0) == INVALID and call(C=9) == INVALID and call(C=-3) == INVALID
    assert call(S=-1) == INVALID and call(nv=0) == INVALID and call(nz=0) == INVALID and call(nz=-2) == INVALID
    for name in none:
        assert call(**{name: None}) == INVALID, name
    assert call(S=1 << 30, nz=4) == INVALID and b"range" in lib.gbp_last_error()
    assert b"gbp_hitmap_pool" in lib.gbp_last_error()


def _hand_made(S=3, C=3):
    """A dict of host tensors by the sampler's names, 3 soundings x 3 chains: per-chain rows carry their own row number."""
    R = S * C
    ident = torch.arange(R, dtype=torch.float64)
    return dict(best_posterior=torch.tensor([1.0, 5.0, 5.0, 2.0, 9.0, 3.0, 7.0, 7.0, 8.0], dtype=torch.float64),
                status=torch.tensor([1, 1, 1, 1, 2, 1, 2, 2, 2], dtype=torch.int32),
                k_hist=torch.arange(R * 4, dtype=torch.int32).view(R, 4), rel_hist=torch.ones((R, 1, 5), dtype=torch.int32),
                first_none=torch.arange(R, dtype=torch.int32).view(R, 1), misfit=ident.clone(), best_sigma=ident[:, None].repeat(1, 2),
                nl_a=torch.arange(3 * R, dtype=torch.int32).view(3, R), add_scale=torch.ones(R, dtype=torch.float64), hitmap=None)


def test_pooled_representative_and_sums_on_a_hand_made_block():
    t = _hand_made()
    p = replicates.Pooled(t, 3)
    assert p.B == 3 and p.use.tolist() == [[True, True, True], [True, False, True], [False, False, False]]
    # sounding 0: chains 1 and 2 tie at 5 -> the lower; sounding 1: the best chain failed -> the best of the used; sounding 2: none -> 0
    assert p.rep.tolist() == [1, 2, 0] and p.rep_rows.tolist() == [1, 5, 6]
    assert p.t["misfit"].tolist() == [1.0, 5.0, 6.0] and p.misfit is p.t["misfit"]
    assert p.t["best_sigma"].tolist() == [[1.0, 1.0], [5.0, 5.0], [6.0, 6.0]] and p.t["status"].tolist() == [1, 1, 2]
    assert "nl_a" not in p.t and p.t["edges"] is None              # working state is not part of the view; absent state stays None
    assert p.t["add_scale"] is t["add_scale"]                       # shared by every row: left alone
    k = t["k_hist"].view(3, 3, 4)
    assert p.t["k_hist"].dtype == torch.int32
    assert torch.equal(p.t["k_hist"], torch.stack([k[0].sum(0), (k[1, 0] + k[1, 2]).to(torch.int64), torch.zeros(4, dtype=torch.int64)]).to(torch.int32))
    assert p.t["rel_hist"][:, 0, 0].tolist() == [3, 2, 0] and p.t["first_none"][:, 0].tolist() == [0 + 1 + 2, 3 + 5, 0]
    assert p.hitmap is None
    # without the reference's schedule every chain is used
    q = replicates.Pooled(t, 3, reference_schedule=False)
    assert bool(q.use.all()) and q.rep.tolist() == [1, 1, 2] and q.t["rel_hist"][:, 0, 0].tolist() == [3, 3, 3]
    with pytest.raises(ValueError):
        replicates.Pooled(t, 2)                                     # 9 chains are not 2 per sounding


def test_command_line_parses_replicates():
    from geobipy_amd.__main__ import parse
    assert parse(["opts", "out"]).replicates == 1 and parse(["opts", "out", "--replicates", "4"]).replicates == 4
    for bad in (["--replicates", "0"], ["--replicates", "9"], ["--replicates", "2", "--no-hitmap"]):
        with pytest.raises(SystemExit):
            parse(["opts", "out"] + bad)


def test_infer_refuses_replicates_it_cannot_run():
    with pytest.raises(ValueError):
        survey.infer(OPTIONS, replicates=0)
    with pytest.raises(ValueError):
        survey.infer(OPTIONS, replicates=2, hitmap=False)
    with pytest.raises(NotImplementedError, match="per-row state"):
        survey.infer(os.path.join(GOLDEN, "skytem_options_small"), replicates=2)


# -- the kernel against the host rule ------------------------------------------------------------------------------------------------

def _planted(C, S=3, nv=7, nz=300, seed=0):
    """Random sparse counts with the corner cases planted in sounding 0 (columns 0 .. 4) and a chain of sounding 1 switched off."""
    rng = np.random.default_rng(seed + C)
    h = (rng.integers(0, 60, size=(S * C, nv, nz)) * (rng.random((S * C, nv, nz)) < 0.5)).astype(np.int32)
    h[0:C, :, 0] = 0                                                # an all-empty column
    h[0, :, 1] = 0                                                  # a used chain with an empty column
    h[0:C, :, 2] = 0
    h[0:C, 3, 2] = 5 + np.arange(C)                                 # W = 0 = Bn: every chain in the bin whose centre is exactly 0
    h[0:C, :, 3] = 0
    for c in range(C):
        h[c, c % nv, 3] = 8                                         # W = 0 < Bn: one bin each, 2^k counts keep every product exact
    h[0, :, 4] = 0
    h[0, 5, 4] = 1                                                  # an n_c = 1 chain
    use = np.ones((S, C), dtype=np.int32)
    use[1, 1] = 0                                                   # a chain switched off
    return h, use


def _compare(out, ref):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["pooled"], ref["pooled"]) and got["pooled"].dtype == np.int32
    assert np.array_equal(got["n_used"], ref["n_used"]) and got["n_used"].dtype == np.int32
    for k in ("rhat", "jsd", "chain_mean"):
        assert got[k].shape == ref[k].shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        assert np.array_equal(np.isposinf(got[k]), np.isposinf(ref[k])) and not np.isneginf(got[k]).any(), k
    for k in ("chain_mean", "rhat"):
        f = np.isfinite(ref[k])
        err = np.abs(got[k][f] - ref[k][f]) / np.maximum(np.abs(ref[k][f]), np.finfo(np.float64).tiny)
        print(k, "largest relative error", err.max() if err.size else 0.0)
        assert np.all(np.abs(got[k][f] - ref[k][f]) <= 1e-12 * np.abs(ref[k][f])), k
    f = np.isfinite(ref["jsd"])
    print("jsd largest absolute error (bits)", np.abs(got["jsd"][f] - ref["jsd"][f]).max() if f.any() else 0.0)
    assert np.all(np.abs(got["jsd"][f] - ref["jsd"][f]) <= 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_kernel_matches_the_host_rule(C):
    from geobipy_amd import hitmap
    h, use = _planted(C)
    ref = replicates.pool_reference(h, C, use, 1.7)
    # the planted cases are what they were planted as
    assert ref["n_used"][0, 0] == 0 and ref["n_used"][0, 1] == C - 1 and ref["n_used"][1].max() == C - 1
    assert ref["rhat"][0, 2] == 1.0 and ref["rhat"][0, 3] == np.inf and ref["n_used"][0, 4] == C
    if C <= 7:                                                      # (C = 8: chains 0 and 7 share a bin)
        assert abs(ref["jsd"][0, 3] - math.log2(C)) <= 1e-12
    out = hitmap.pool(torch.as_tensor(h).cuda(), C, torch.as_tensor(use).cuda(), 1.7)
    _compare(out, ref)
    # use=None: every chain
    _compare(hitmap.pool(torch.as_tensor(h).cuda(), C, None, 1.7), replicates.pool_reference(h, C, None, 1.7))


@pytest.mark.gpu
def test_pooled_map_at_the_survey_shape_feeds_the_products():
    from geobipy_amd import hitmap
    S, C, nv, nz = 4, 4, 250, 440
    g = torch.Generator().manual_seed(5)
    h = (torch.randint(0, 3000, (S * C, nv, nz), generator=g, dtype=torch.int32) * (torch.rand((S * C, nv, nz), generator=g) < 0.1)).to(torch.int32).cuda()
    use = torch.ones((S, C), dtype=torch.int32)
    use[2, 3] = 0
    out = hitmap.pool(h, C, use.cuda(), 2.1)
    want = (h.view(S, C, nv, nz) * use.cuda()[:, :, None, None]).sum(dim=1).to(torch.int32)
    assert torch.equal(out["pooled"], want)
    lmp = torch.linspace(-3.0, -1.0, S, dtype=torch.float64).cuda()
    a, b = hitmap.products(out["pooled"], lmp, 2.1), hitmap.products(want, lmp, 2.1)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k],
                           b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k]), k
    # the pooled column's mean is the sample-weighted mean of the chains' means
    n = h.view(S, C, nv, nz).sum(dim=2).to(torch.float64) * use.cuda()[:, :, None]
    mix = (torch.nan_to_num(out["chain_mean"]) * n).sum(dim=1) / n.sum(dim=1)
    shift = lmp[:, None] / math.log(10.0)
    assert torch.allclose(a["mean"] - shift, mix, rtol=0.0, atol=1e-10)


@pytest.mark.gpu
def test_generic_axis_layer_count_histograms():
    from geobipy_amd import hitmap
    rng = np.random.default_rng(3)
    S, C, K = 5, 3, 30
    k_hist = rng.integers(0, 500, size=(S * C, K + 1)).astype(np.int32)
    k_hist[:, 0] = 0
    k_hist[C:2 * C, 12:] = 0
    use = np.ones((S, C), dtype=np.int32)
    use[3] = [1, 0, 0]
    out = hitmap.pool(torch.as_tensor(k_hist).cuda()[:, :, None], C, torch.as_tensor(use).cuda(), 1.0)
    ref = replicates.pool_reference(k_hist[:, :, None], C, use, 1.0)
    assert out["rhat"].shape == (S, 1) and out["pooled"].shape == (S, K + 1, 1)
    _compare(out, ref)
    assert np.isnan(ref["rhat"][3, 0]) and np.isfinite(ref["rhat"][[0, 1, 2, 4], 0]).all()


# -- chains --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_replicate_zero_is_the_plain_chain_and_the_pool_counts_every_sample():
    from geobipy_amd.rjmcmc_gpu import DeviceChains
    o = survey.read_options(OPTIONS, n_markov_chains=1500)
    ds = survey.FdemData.read_csv(o["data_filename"], o["system_filename"])
    rows, C = np.array([2, 30, 31, 60, 78]), 3
    kw = dict(seed=11, hitmap=True, reference_schedule=True, burn_in_min_iterations=300, **{k: o[k] for k in CHAIN_KEYS if o.get(k) is not None})
    plain = DeviceChains(ds.system, ds.z[rows], ds.data[rows], chain_id=rows, **kw)
    plain.infer(check_every=500)
    rep, cid = replicates.expand(rows, C, ds.nPoints)
    dc = DeviceChains(ds.system, ds.z[rep], ds.data[rep], chain_id=cid, **kw)
    dc.infer(check_every=500)
    hm, hm0 = dc.hitmap.view(rows.size, C, dc.n_value_bins, dc.n_depth_bins), plain.hitmap
    assert torch.equal(hm[:, 0], hm0) and torch.equal(dc.t["k_hist"][0::C], plain.t["k_hist"])
    for k in ("best_k", "best_sigma", "best_edges", "best_posterior", "status", "burned_in_iteration"):
        assert torch.equal(dc.t[k][0::C], plain.t[k]), k
    assert not torch.equal(hm[:, 1], hm[:, 0]) and not torch.equal(hm[:, 2], hm[:, 0]) and not torch.equal(hm[:, 2], hm[:, 1])
    p = replicates.Pooled(dc, C)
    assert torch.equal(p.use, (dc.t["status"] != 2).view(rows.size, C)) and bool(p.use.any())
    samples = (dc.t["k_hist"].sum(dim=1).view(rows.size, C) * p.use).sum(dim=1)      # one count per accumulated model ...
    totals = (hm.sum(dim=2, dtype=torch.int64) * p.use[:, :, None]).sum(dim=1)       # ... in a depth cell of the chain's hit map
    assert torch.equal(p.hitmap.sum(dim=1, dtype=torch.int64), totals) and torch.equal(totals[:, 0], samples)
    assert torch.equal(p.t["k_hist"].sum(dim=1, dtype=torch.int64), samples)
    d = p.diagnostics()
    S, nz = rows.size, dc.n_depth_bins
    assert d["rhat"].shape == (S, nz) and d["jsd"].shape == (S, nz) and d["n_used"].shape == (S, nz) and d["chain_mean"].shape == (S, C, nz)
    for k in ("rhat_layers", "jsd_layers", "rhat_interfaces", "rhat_max"):
        assert d[k].shape == (S,), k
    assert torch.equal(d["n_used"][:, 0], p.use.sum(dim=1).to(torch.int32))
    two = p.use.sum(dim=1) >= 2
    assert bool(((d["jsd"][two] >= 0.0) & (d["jsd"][two] <= math.log2(C) + 1e-12)).all())
    ref = replicates.pool_reference(dc.t["k_hist"].cpu().numpy()[:, :, None], C, p.use.cpu().numpy(), 1.0)
    assert np.allclose(d["rhat_layers"].cpu().numpy(), ref["rhat"][:, 0], rtol=1e-12, atol=0.0, equal_nan=True)
    # the representative chain: the highest posterior among the used
    score = torch.where(p.use, dc.t["best_posterior"].view(S, C), torch.full((), float("-inf"), dtype=torch.float64, device=p.use.device))
    assert torch.equal(p.t["best_posterior"], torch.where(p.use.any(dim=1), score.max(dim=1).values, dc.t["best_posterior"][0::C]))


def _container(directory, line):
    from geobipy_amd import hdf
    path = hdf.results_path(str(directory), line)
    return hdf.load_results(path if path.endswith(".h5") else path + ".npz")[0]


@pytest.mark.gpu
def test_survey_with_replicates_fills_the_containers_from_the_pool(tmp_path):
    from geobipy_amd import intervals, unit_posteriors
    from geobipy_amd.rjmcmc_gpu import DeviceChains
    C = 2
    out1, out2 = tmp_path / "one", tmp_path / "two"
    out1.mkdir()
    out2.mkdir()
    spec = {"kind": "depth", "edges": [0.0, 10.0, 30.0, 75.0]}       # sampled unit posteriors ride along: summed over the used chains
    one = survey.infer(OPTIONS, exact_jacobian=True, results_directory=str(out1), replicates=1, units=spec, first_above=(0.1,), **SHORT)
    res = survey.infer(OPTIONS, exact_jacobian=True, results_directory=str(out2), replicates=C, units=spec, first_above=(0.1,), **SHORT)
    # the same chains through DeviceChains and Pooled
    o = survey.read_options(OPTIONS, n_markov_chains=SHORT["n_markov_chains"])
    ds = survey.FdemData.read_csv(o["data_filename"], o["system_filename"])
    rep, cid = replicates.expand(np.arange(ds.nPoints), C, ds.nPoints)
    dc = DeviceChains(ds.system, ds.z[rep], ds.data[rep], seed=int(o["seed"]) % (1 << 64), exact_jacobian=True, hitmap=True, chain_id=cid,
                      reference_schedule=True, burn_in_min_iterations=SHORT["burn_in_min_iterations"],
                      units=intervals.unit_bounds(spec, ds.nPoints, max_depth=1.1 * o["maximum_depth"])[rep], first_above=(0.1,),
                      **{k: o[k] for k in CHAIN_KEYS if o.get(k) is not None})
    dc.infer(check_every=SHORT["check_every"])
    p = replicates.Pooled(dc, C)
    # the sampled unit posteriors of the pooled view: the used chains' histograms added up, and the statistics of that sum in the summaries
    for name in ("unit_hist", "first_hist", "first_none"):
        full = getattr(dc, name)
        mask = p.use.view((ds.nPoints, C) + (1,) * (full.ndim - 1))
        assert torch.equal(p.t[name], (full.view((ds.nPoints, C) + tuple(full.shape[1:])) * mask).sum(dim=1).to(torch.int32)), name
    assert int(p.t["unit_hist"].sum()) > 0 and torch.equal(p.t["unit_z"], dc.t["unit_z"][0::C])
    for k, v in unit_posteriors.products(p).items():
        v = v.cpu().numpy()
        assert np.array_equal(res[k], v[:, 0] if v.shape[1] == 1 else v, equal_nan=True), k
    d = {k: v.cpu().numpy() for k, v in p.diagnostics().items()}
    S, nz = ds.nPoints, dc.n_depth_bins
    # the summaries: the diagnostics, with their shapes
    assert set(res) - set(one) == set(survey.REPLICATE_SUMMARIES) | {"replicates_used"} and set(one) <= set(res)
    assert res["rhat"].shape == (S, nz) and res["jsd"].shape == (S, nz) and res["n_used"].shape == (S, nz) and res["chain_mean"].shape == (S, C, nz)
    for k in ("rhat_layers", "jsd_layers", "rhat_interfaces", "rhat_max", "replicates_used"):
        assert res[k].shape == (S,), k
    for k in survey.REPLICATE_SUMMARIES:
        assert np.array_equal(res[k], d[k], equal_nan=True), k
    assert np.array_equal(res["replicates_used"], p.use.sum(dim=1).cpu().numpy()) and res["n_used"].dtype == np.int64
    assert np.array_equal(res["layer_count_posterior"], p.t["k_hist"].cpu().numpy())
    assert np.array_equal(res["best_posterior"], p.t["best_posterior"].cpu().numpy())
    # replicate 0 is the chain of the run without replicates: where it alone is used, the pooled posterior contains it
    assert np.all(res["layer_count_posterior"].sum(axis=1) >= np.where(one["status"] != 2, one["layer_count_posterior"].sum(axis=1), 0))
    # the containers: the reference's layout, the pooled hit maps
    hm = p.hitmap.cpu().numpy()
    for ln in np.unique(ds.lineNumber):
        z1, z2 = _container(out1, ln), _container(out2, ln)
        assert sorted(z1) == sorted(z2)
        for k in z1:
            assert z1[k].shape == z2[k].shape and z1[k].dtype == z2[k].dtype, k
        m = ds.lineNumber == ln
        rows_ = np.nonzero(m)[0][np.argsort(ds.fiducial[m])]
        assert np.array_equal(z2["/model/values/posterior/values/data"], hm[rows_])
        assert np.array_equal(z2["/model/mesh/nCells/posterior/values/data"], res["layer_count_posterior"][rows_])
        assert np.array_equal(z2["/model/mesh/nCells/data"], res["best_n_layers"][rows_])
    # the per-line summary files carry the diagnostics
    paths = res.save_lines(str(tmp_path))
    line = np.load(paths[0])
    first = ds.lineNumber == np.unique(ds.lineNumber)[0]
    assert np.array_equal(line["rhat"], res["rhat"][first], equal_nan=True) and line["chain_mean"].shape == (int(first.sum()), C, nz)


@pytest.mark.gpu
def test_one_replicate_is_the_run_without_the_argument():
    plain = survey.infer(OPTIONS, exact_jacobian=True, **SHORT)
    one = survey.infer(OPTIONS, exact_jacobian=True, replicates=1, **SHORT)
    assert set(plain) == set(one) and "rhat" not in one
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(one[k]), equal_nan=True), k
