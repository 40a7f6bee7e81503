"""Sampled unit posteriors on the device (csrc/gbp_rjmcmc.h units_add; rjmcmc_gpu.DeviceChains(units=..., first_above=..., first_below=...))
against the host rule inference.Posteriors(units=..., first=...): integer equality with a host replay of the chains' states, the
invariants that tie the histograms to the layer-count posterior, the same counts from every driver and sharding, time-domain chains,
no influence on the chains themselves, and the summaries of a survey run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import unit_posteriors
from test_rjmcmc_gpu import GOLDEN, _chains

# 8 depth units: one empty (dz == 0), one thinner than a depth cell, one over the whole depth axis, one reaching far past the deepest
# interface the prior allows (maximum_depth 200 m)
UNITS = np.array([[0.0, 10.0], [10.0, 30.0], [30.0, 75.0], [5.0, 5.0], [0.0, 200.0], [2.5, 2.75], [75.0, 150.0], [120.0, 1000.0]])
# the golden sounding's half-space is 0.067 S/m: layers at or above 0.1 S/m and at or below 0.03 S/m both occur, neither always
FIRST = dict(first_above=(0.1,), first_below=(0.03,))
UNIT_KW = dict(hitmap=True, units=UNITS, unit_kinds=("arithmetic", "harmonic"), **FIRST)
EDGE = 1.0e-9               # fractional bin positions this close to an integer may round the other way with the device's logarithm
CAP = 0.001                 # ... for at most this fraction of the samples


def _host_posteriors(dc, units=UNITS, nv=None):
    from geobipy_amd.inference import Posteriors
    o = dc.o
    lmp = dc.log_mean_prior.cpu().numpy()
    posts = []
    for b in range(dc.B):
        p = Posteriors(dc.K, o["maximum_depth"], o["minimum_thickness"], float(np.exp(lmp[b])), o["factor"],
                       n_value_bins=dc.n_value_bins if nv is None else nv, units=units if np.ndim(units) == 2 else units[b],
                       unit_kinds=dc.unit_kinds, first=(dc.first_threshold, dc.first_direction))
        p.log_mean_prior = np.float64(lmp[b])                    # the chain's own value, not log(exp(.)) of it
        assert p.value_half_width == np.float64(dc.value_half_width) and p.depth_bin_width == np.float64(dc.depth_bin_width)
        posts.append(p)
    return posts


def _states(dc):
    return dc.k.cpu().numpy(), dc.edges.cpu().numpy(), dc.sigma.cpu().numpy()


def _compare_with_replay(dc, posts, n_samples):
    """unit_hist / first_hist / first_none of the device == the host replay, as integers; a (chain, kind, unit) column is left out when
    one of its samples sat within EDGE of a bin edge on the host.  Returns the number of samples left out (asserted against CAP)."""
    uh = dc.unit_hist.cpu().numpy()
    left_out = 0
    for b, p in enumerate(posts):
        near = {(q, m) for q, m, d in p.unit_edge_distance if d < EDGE}
        left_out += sum(1 for q, m, d in p.unit_edge_distance if (q, m) in near)
        for q in range(uh.shape[1]):
            for m in range(uh.shape[3]):
                if (q, m) not in near:
                    assert np.array_equal(uh[b, q, :, m], p.unit_hist[q, :, m]), (b, q, m)
    print("host replay: %d of %d unit samples left out (within %g of a bin edge); cap %d" % (left_out, n_samples, EDGE, int(CAP * n_samples)))
    assert left_out <= CAP * n_samples
    assert np.array_equal(dc.first_hist.cpu().numpy(), np.stack([p.first_hist for p in posts]))
    assert np.array_equal(dc.first_none.cpu().numpy(), np.stack([p.first_none for p in posts]))
    return left_out


def test_unit_posteriors_match_a_host_replay_and_keep_their_invariants():
    B, n_acc = 16, 150
    _, _, dc = _chains(B, 4, exact=True, **UNIT_KW)
    assert dc.unit_hist.shape == (B, 2, dc.n_value_bins, 8) and dc.first_hist.shape == (B, 2, dc.n_depth_bins) and dc.first_none.shape == (B, 2)
    dc.run(200, accumulate=False)
    assert int(dc.unit_hist.sum()) == 0 and int(dc.first_hist.sum()) == 0 and int(dc.first_none.sum()) == 0 and int(dc.hitmap.sum()) == 0
    posts = _host_posteriors(dc)
    for _ in range(n_acc):
        dc.step()
        k, e, s = _states(dc)
        for b in range(B):
            posts[b].update(e[b, : k[b] - 1], s[b, : k[b]])
    _compare_with_replay(dc, posts, B * n_acc * 8)                # 19 200 samples (16 chains x 150 states x 8 units): at most 19 left out
    assert np.array_equal(dc.hitmap.cpu().numpy(), np.stack([p.values for p in posts]))       # the hit map of the same run: still exact
    assert np.array_equal(dc.k_hist.cpu().numpy(), np.stack([p.n_cells for p in posts]))
    # invariants
    total = dc.k_hist.sum(dim=1).cpu().numpy()
    assert np.all(total == n_acc)
    uh, fh, fn = dc.unit_hist.cpu().numpy().astype(np.int64), dc.first_hist.cpu().numpy().astype(np.int64), dc.first_none.cpu().numpy()
    dz = UNITS[:, 1] - UNITS[:, 0]
    per_unit = uh.sum(axis=2)                                     # [B, Q, M]
    assert np.all(per_unit[:, :, dz > 0] == total[:, None, None]) and np.all(per_unit[:, :, dz == 0] == 0)
    assert np.array_equal(fh.sum(axis=2) + fn, np.broadcast_to(total[:, None], fn.shape))
    assert fh.sum() > 0 and fn.sum() > 0
    cum = np.cumsum(uh, axis=2)
    assert np.all(cum[:, 1] >= cum[:, 0])                         # harmonic <= arithmetic, sample by sample
    assert np.any(cum[:, 1] > cum[:, 0])
    # the statistics: shapes, NaN for the empty unit, h <= a, conductance = arithmetic + log10 dz
    out = unit_posteriors.products(dc)
    a, h = out["unit_arithmetic_median"].cpu().numpy(), out["unit_harmonic_median"].cpu().numpy()
    assert a.shape == (B, 8) and np.isnan(a[:, 3]).all() and not np.isnan(np.delete(a, 3, axis=1)).any()
    assert np.all(np.delete(h, 3, axis=1) <= np.delete(a, 3, axis=1))
    live_m = dz > 0
    assert np.allclose(out["unit_conductance_median"].cpu().numpy()[:, live_m], a[:, live_m] + np.log10(dz[live_m]), atol=1e-12, rtol=0)
    assert np.allclose(out["unit_resistance_percentile_5"].cpu().numpy()[:, live_m],
                       np.log10(dz[live_m]) - out["unit_harmonic_percentile_95"].cpu().numpy()[:, live_m], atol=1e-12, rtol=0)
    assert out["first_depth_median"].shape == (B, 2) and out["first_probability"].shape == (B, 2)
    assert np.allclose(out["first_probability"].cpu().numpy(), 1.0 - fn / total[:, None])
    # a unit inside the whole-axis unit of a half-space model would be that layer: here, the statistics of hand-made histograms
    hand = torch.zeros((2, 2, dc.n_value_bins, 3), dtype=torch.int32, device=dc.device)
    hand[:, 0, 100, :] = 7; hand[:, 1, 60, :] = 7; hand[1, :, :, 2] = 0
    lmp = torch.log(torch.tensor([0.1, 0.01], dtype=torch.float64))
    z = torch.tensor([[0.0, 10.0], [10.0, 110.0], [7.0, 7.0]], dtype=torch.float64).expand(2, 3, 2)
    got = unit_posteriors.products(dict(unit_hist=hand, log_mean_prior=lmp, unit_z=z, value_half_width=dc.value_half_width,
                                        depth_bin_width=dc.depth_bin_width, unit_kinds=("arithmetic", "harmonic")))
    centre = lambda i, mean: (i + 0.5) / dc.n_value_bins * 2 * dc.value_half_width - dc.value_half_width + np.log10(mean)      # noqa: E731
    am = got["unit_arithmetic_median"].cpu().numpy()
    assert np.allclose(am[:, :2], [[centre(100, 0.1)] * 2, [centre(100, 0.01)] * 2], atol=1e-12) and np.isnan(am[:, 2]).all()
    assert np.allclose(got["unit_conductance_mode"].cpu().numpy()[0, :2], centre(100, 0.1) + np.array([1.0, 2.0]), atol=1e-12)
    assert np.allclose(got["unit_resistance_median"].cpu().numpy()[1, :2], np.array([1.0, 2.0]) - centre(60, 0.01), atol=1e-12)


def _driver_runs(units_kw, n_it=400, B=300):
    """The runs of test_persistent_kernel_walks_the_same_chains's schedule case, with unit posteriors."""
    # (21 value cells where that test has 20: a chain starts from the half-space AT its prior mean, which is a cell edge of an even axis --
    #  there the last bit of a logarithm decides the cell, and the host's is not the device's; an odd axis has it at a cell centre)
    kw = dict(reference_schedule=True, burn_in_min_iterations=60, n_value_bins=21, options=dict(n_markov_chains=150))
    runs = []
    for mode, cuts in ((1, (n_it,)), (2, (n_it,)), (2, (1, 7, 150, n_it - 158)), (4, (n_it,)), (4, (90, n_it - 90))):
        d, s, dc = _chains(B, 31, exact=True, **dict(kw, options=dict(kw["options"])), **units_kw)
        rng = np.random.default_rng(4)
        dc.data.copy_(torch.as_tensor(np.tile(d["data"], (B, 1)) * rng.uniform(0.7, 1.4, (B, 1))))
        dc._initialize()
        dc.run_mode = mode
        for n in cuts:
            dc.run(n)
        torch.cuda.synchronize()
        runs.append(dc)
    return runs


def test_every_driver_accumulates_the_same_unit_posteriors():
    """Lock-step, persistent and concurrent sub-blocks under the reference's schedule (burn-in reset, chains that finish): equal arrays,
    and equal to a host replay of the lock-step run that resets at the recorded burn-in iteration."""
    runs = _driver_runs(dict(UNIT_KW))
    ref = runs[0]
    assert int((ref.status == 1).sum()) > 0 and int((ref.burned_in_iteration > 0).sum()) > 0
    for other in runs[1:]:
        for n in ("k", "sigma", "k_hist", "hitmap", "unit_hist", "first_hist", "first_none", "burned_in_iteration", "status"):
            assert torch.equal(getattr(ref, n), getattr(other, n)), (other.run_mode, n)
    total = ref.k_hist.sum(dim=1)
    live = torch.as_tensor(UNITS[:, 1] > UNITS[:, 0], device=ref.device)
    assert torch.equal(ref.unit_hist.sum(dim=2)[:, :, live].long(), total[:, None, None].expand(-1, 2, int(live.sum())).long())
    assert torch.equal((ref.first_hist.sum(dim=2) + ref.first_none).long(), total[:, None].expand(-1, 2).long())
    # host replay of 24 of the chains, step by step, with the schedule's reset and stop
    B, n_it = 24, 400
    d, s, dc = _chains(B, 31, exact=True, reference_schedule=True, burn_in_min_iterations=60, n_value_bins=21,
                       options=dict(n_markov_chains=150), **UNIT_KW)
    rng = np.random.default_rng(4)
    dc.data.copy_(torch.as_tensor((np.tile(d["data"], (300, 1)) * rng.uniform(0.7, 1.4, (300, 1)))[:B]))
    dc._initialize()
    posts = _host_posteriors(dc)
    done = np.zeros(B, dtype=bool)
    seen_bi = np.full(B, -1)
    n_samples = 0
    for it in range(n_it):
        dc.step()
        k, e, s_ = _states(dc)
        bi, status = dc.burned_in_iteration.cpu().numpy(), dc.status.cpu().numpy()
        for b in range(B):
            if done[b]:
                continue
            if bi[b] >= 0 and seen_bi[b] < 0:                     # burned in at this very iteration: the posteriors start over with it
                posts[b].reset()
                seen_bi[b] = bi[b]
            posts[b].update(e[b, : k[b] - 1], s_[b, : k[b]])
            n_samples += 8
            done[b] = status[b] != 0
    for n in ("k", "sigma", "burned_in_iteration", "status", "unit_hist", "first_hist", "first_none"):
        assert torch.equal(getattr(dc, n), getattr(ref, n)[:B]), n           # (the same chains: keyed by row)
    assert done.any() and (seen_bi > 0).any()
    _compare_with_replay(dc, posts, n_samples)
    assert np.array_equal(dc.hitmap.cpu().numpy(), np.stack([p.values for p in posts]))


def test_a_restart_zeroes_the_unit_posteriors():
    """infer()'s restart of stuck chains (_restart_stuck_chains) starts the unit posteriors over like the hit map."""
    r = np.load(os.path.join(GOLDEN, "mcmc_reset.npz"))
    window, reset_limit, n_mc = (int(x) for x in r["stuck1_meta"][:3])
    s0 = float(np.sqrt(np.prod(r["stuck1_limits"])))
    B = 8
    _, _, dc = _chains(B, 5, exact=True, reference_schedule=True, **UNIT_KW,
                       options=dict(n_markov_chains=n_mc, update_plot_every=window, reset_limit=reset_limit,
                                    parameter_limits=[s0 * (1.0 - 1e-9), s0 * (1.0 + 1e-9)]))
    dc.run(window - 1)
    assert int(dc.unit_hist.sum()) > 0 and int(dc.first_hist.sum() + dc.first_none.sum()) > 0
    snap = dc.t["n_accepted"].clone()
    dc.run(1)                                                     # the update that closes the window (infer() does the same)
    dc._restart_stuck_chains(dc.t["status"] == 0, snap, reset_limit)
    assert torch.all(dc.n_resets == 1) and torch.all(dc.iteration0 == window)
    for n in ("unit_hist", "first_hist", "first_none", "hitmap", "hit_dwell"):
        assert int(dc.t[n].abs().sum()) == 0, n
    dc.run(5)                                                     # ... and they fill again from the restart
    assert int(dc.unit_hist.sum()) == B * 5 * 14 and int((dc.first_hist.sum(dim=2) + dc.first_none).sum()) == B * 5 * 2


def test_sharding_does_not_change_the_unit_posteriors():
    B, half = 64, 32
    bounds = np.tile(UNITS, (B, 1, 1))
    bounds[:, 1, 1] += np.arange(B)                               # per-sounding bounds: the rows must travel with their chains
    kw = dict(UNIT_KW, units=None)
    d, s, whole = _chains(B, 9, **dict(kw, units=bounds), first_chain=1000)
    whole.run(120)
    for first in (0, half):
        _, _, part = _chains(half, 9, **dict(kw, units=bounds[first:first + half]), first_chain=1000 + first)
        part.run(120)
        for n in ("k", "sigma", "k_hist", "hitmap", "unit_hist", "first_hist", "first_none"):
            assert torch.equal(getattr(whole, n)[first:first + half], getattr(part, n)), (first, n)
    assert int(whole.n_accepted.sum()) > B and int(whole.unit_hist.sum()) == B * 120 * 14


def test_unit_posteriors_do_not_perturb_the_chains():
    """Feature off: the chains and hit maps of a run without units equal those of the same seeds with units, in every driver."""
    for mode in (1, 2):
        runs = []
        for kw in (dict(hitmap=True), dict(UNIT_KW)):
            _, _, dc = _chains(96, 21, **kw)
            dc.run_mode = mode
            dc.run(50, accumulate=False)
            dc.run(150)
            runs.append(dc)
        off, on = runs
        assert off.t["unit_hist"] is None and off.t["first_hist"] is None and off._o.n_units == 0
        for n in ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "n_accepted", "k_hist", "edge_hist", "hitmap",
                  "best_posterior", "best_sigma", "log_ratio"):
            assert torch.equal(getattr(off, n), getattr(on, n)), (mode, n)
        assert int(on.unit_hist.sum()) == 96 * 150 * 14


def test_unit_arguments_are_checked_before_any_launch():
    from geobipy_amd import _lib
    with pytest.raises(ValueError, match="hitmap"):
        _chains(4, 1, units=UNITS)                                # no hit map
    with pytest.raises(ValueError):
        _chains(4, 1, hitmap=True, units=[[5.0, 1.0]])
    with pytest.raises(ValueError):
        _chains(4, 1, hitmap=True, first_above=(0.1, 0.2, 0.3), first_below=(0.1, 0.2))
    _, _, dc = _chains(4, 1, **UNIT_KW)
    lib = _lib.load()
    for field, value in (("unit_kinds", 0), ("unit_kinds", 4), ("n_units", 17), ("n_first", 5)):
        o = _lib.RjOptions.from_buffer_copy(dc._o)
        setattr(o, field, value)
        assert lib.gbp_rj_run_mode(dc._h.ptr, o, dc._c, 0, 1, 1, 1, dc._stream()) != 0, field
    o = _lib.RjOptions.from_buffer_copy(dc._o)
    o.first_threshold[0] = float("nan")
    assert lib.gbp_rj_run_mode(dc._h.ptr, o, dc._c, 0, 1, 1, 1, dc._stream()) != 0
    o = _lib.RjOptions.from_buffer_copy(dc._o)
    o.first_direction[1] = 0
    assert lib.gbp_rj_run_mode(dc._h.ptr, o, dc._c, 0, 1, 1, 1, dc._stream()) != 0
    c = _lib.RjChains.from_buffer_copy(dc._c)
    c.hitmap = None
    assert lib.gbp_rj_run_mode(dc._h.ptr, dc._o, c, 0, 1, 1, 1, dc._stream()) != 0
    assert b"hit map" in lib.gbp_last_error()
    assert int(dc.k_hist.sum()) == 0                              # nothing ran


def test_time_domain_chains_accumulate_unit_posteriors():
    from geobipy_amd.tdem import TdemDeviceChains
    from test_tdem_sampler import OFFSET, _survey
    B, n_acc = 4, 120
    s, h, data, scale, opts, groups = _survey(B, seed=3)          # the golden SkyTEM low-moment system
    units = np.array([[0.0, 15.0], [15.0, 60.0], [60.0, 60.0], [40.0, 2000.0]])
    dc = TdemDeviceChains(s, h, data, OFFSET, seed=77, hitmap=True, units=units, first_above=(0.03,), first_below=(0.01,), **opts)
    dc.run(100, accumulate=False)
    posts = _host_posteriors(dc, units)
    for _ in range(n_acc):
        dc.step()
        k, e, sg = _states(dc)
        for b in range(B):
            posts[b].update(e[b, : k[b] - 1], sg[b, : k[b]])
    assert int(dc.n_accepted.sum()) > 0
    _compare_with_replay(dc, posts, B * n_acc * 4)
    assert np.array_equal(dc.hitmap.cpu().numpy(), np.stack([p.values for p in posts]))


def test_survey_summaries_carry_the_unit_statistics(tmp_path):
    """survey.infer(units=...): the unit statistics join the per-sounding summaries and equal unit_posteriors.products on a DeviceChains
    run of the same seeds; the command line's --units-depth / --first-above write them into the summary files."""
    from geobipy_amd import intervals, survey
    from geobipy_amd.__main__ import main
    from geobipy_amd.survey import FdemData, read_options
    options = os.path.join(GOLDEN, "resolve_options_small")
    spec = dict(kind="depth", edges=[0.0, 10.0, 30.0, 75.0])
    res = survey.infer(options, exact_jacobian=True, units=spec, first_above=(0.1,))
    N = res["status"].size
    for k in ("unit_arithmetic_mean", "unit_harmonic_median", "unit_conductance_percentile_5", "unit_resistance_percentile_95",
              "unit_arithmetic_credible_range", "unit_thickness"):
        assert res[k].shape == (N, 3), k
    assert res["first_depth_median"].shape == (N,) and res["first_probability"].shape == (N,)
    assert np.array_equal(res["unit_thickness"], np.tile([10.0, 20.0, 45.0], (N, 1)))
    done = res["status"] == 1
    assert done.any() and not np.isnan(res["unit_arithmetic_mean"][done]).any()
    assert np.all(res["unit_harmonic_median"][done] <= res["unit_arithmetic_median"][done])
    # the same chains through DeviceChains
    o = read_options(options)
    ds = FdemData.read_csv(o["data_filename"], o["system_filename"])
    plain = survey.infer(options, exact_jacobian=True)
    for k in ("status", "n_layers", "misfit", "mean_log10_conductivity"):
        assert np.array_equal(res[k], plain[k], equal_nan=True), k       # accumulating the units changes no chain
    from geobipy_amd.rjmcmc_gpu import DeviceChains
    keys = ("n_markov_chains", "solve_gradient", "maximum_number_of_layers", "minimum_depth", "maximum_depth", "minimum_thickness",
            "initial_relative_error", "minimum_relative_error", "maximum_relative_error", "initial_additive_error", "minimum_additive_error",
            "maximum_additive_error", "relative_error_proposal_variance", "additive_error_proposal_variance", "probability_of_birth",
            "probability_of_death", "probability_of_perturb", "probability_of_no_change", "factor", "gradient_standard_deviation",
            "covariance_scaling", "parameter_limits", "update_plot_every", "reset_limit", "solve_parameter", "solve_relative_error",
            "solve_additive_error")
    dc = DeviceChains(ds.system, ds.z, ds.data, seed=o.get("seed", 0), exact_jacobian=True, hitmap=True, first_chain=0, reference_schedule=True,
                      units=intervals.unit_bounds(spec, ds.nPoints, max_depth=1.1 * o["maximum_depth"]), first_above=(0.1,),
                      **{k: o[k] for k in keys if o.get(k) is not None})
    dc.infer()
    assert np.array_equal(dc.status.cpu().numpy(), res["status"])
    for k, v in unit_posteriors.products(dc).items():
        v = v.cpu().numpy()
        assert np.array_equal(res[k], v[:, 0] if v.shape[1] == 1 else v, equal_nan=True), k
    # the command line
    out = tmp_path / "cli"
    out.mkdir()
    assert main([options, str(out), "--exact-jacobian", "--no-containers", "--units-depth", "0", "10", "30", "75", "--first-above", "0.1"]) == 0
    ln = np.unique(res["line"])[0]
    line = np.load(str(out / "{}.npz".format(ln)))
    assert np.array_equal(line["unit_conductance_median"], res["unit_conductance_median"][res["line"] == ln], equal_nan=True)
    assert "first_depth_percentile_5" in line.files and "unit_resistance_mean" in line.files
