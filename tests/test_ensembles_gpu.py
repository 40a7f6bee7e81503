"""Posterior ensembles on the device (csrc/gbp_rjmcmc.h ensemble_add; csrc/gbp_ensemble.h; rjmcmc_gpu.DeviceChains(ensemble=...);
geobipy_amd.ensembles) against the host rule inference.Posteriors(ensemble=...): bit equality with a host replay of the chains' states,
the same slots from every driver and sharding, the re-binning kernel closing the loop with the sampler's own posteriors, the raster
against numpy, restarts, time-domain chains, no influence on the chains themselves, the refusals, replicates and a survey run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import ensembles
from test_rjmcmc_gpu import GOLDEN, _chains

ENS = ("ens_k", "ens_edges", "ens_sigma", "ens_misfit", "ens_seen")


def _host_posteriors(dc):
    from geobipy_amd.inference import Posteriors
    o, lmp = dc.o, dc.log_mean_prior.cpu().numpy()
    return [Posteriors(dc.K, o["maximum_depth"], o["minimum_thickness"], float(np.exp(lmp[b])), o["factor"], n_value_bins=dc.n_value_bins,
                       ensemble=dict(n_keep=dc.n_ensemble, thin=dc.ensemble_thin)) for b in range(dc.B)]


def _states(dc):
    return dc.k.cpu().numpy(), dc.edges.cpu().numpy(), dc.sigma.cpu().numpy(), dc.misfit.cpu().numpy()


def _compare_with_replay(dc, posts):
    """Every filled slot equals the replay's bit for bit, padded with +inf / NaN; empty slots have k == 0; returns the filled counts."""
    k, e, s, m, seen = (getattr(dc, n).cpu().numpy() for n in ENS)
    hk = np.stack([p.ens_k for p in posts])
    assert np.array_equal(k, hk)
    assert np.array_equal(seen, [p.ens_seen for p in posts])
    filled = k > 0
    he, hs, hm = (np.stack([getattr(p, n) for p in posts]) for n in ("ens_edges", "ens_sigma", "ens_misfit"))
    assert np.array_equal(e[filled].view(np.int64), he[filled].view(np.int64))        # the doubles' bits, +inf padding included
    assert np.array_equal(np.isnan(s[filled]), np.isnan(hs[filled]))                   # NaN padding exactly past the k conductivities
    live = ~np.isnan(hs[filled])
    assert np.array_equal(s[filled][live].view(np.int64), hs[filled][live].view(np.int64))
    assert np.array_equal(m[filled].view(np.int64), hm[filled].view(np.int64))
    cols = np.arange(e.shape[2])[None, :]
    assert np.all(np.isposinf(e[filled]) == (cols >= k[filled][:, None] - 1)) and np.all(np.isnan(s[filled]) == (cols >= k[filled][:, None]))
    return filled.sum(axis=1)


@pytest.mark.parametrize("thin, n_keep, n_filled", [(3, 64, 50), (2, 40, 40)])
def test_the_ensemble_matches_a_host_replay(thin, n_keep, n_filled):
    B, n_acc = 16, 150
    _, _, dc = _chains(B, 4, exact=True, hitmap=True, ensemble=dict(n_keep=n_keep, thin=thin))
    K = dc.K
    assert dc.t["ens_k"].shape == (B, n_keep) and dc.t["ens_edges"].shape == (B, n_keep, K) and dc.t["ens_sigma"].shape == (B, n_keep, K)
    assert dc.t["ens_misfit"].shape == (B, n_keep) and dc.t["ens_seen"].shape == (B,) and dc.t["ens_k"].dtype == torch.int32
    dc.run(200, accumulate=False)
    assert int(dc.ens_seen.sum()) == 0 and int(dc.ens_k.sum()) == 0 and int(dc.hitmap.sum()) == 0
    posts = _host_posteriors(dc)
    for _ in range(n_acc):
        dc.step()
        k, e, s, misfit = _states(dc)
        for b in range(B):
            posts[b].update(e[b, : k[b] - 1], s[b, : k[b]], misfit=misfit[b])
    counts = _compare_with_replay(dc, posts)
    assert np.all(counts == n_filled) and np.all(dc.ens_k.cpu().numpy()[:, n_filled:] == 0)       # chain order: the first slots, no holes
    assert np.array_equal(dc.ens_seen.cpu().numpy(), dc.k_hist.sum(dim=1).cpu().numpy()) and np.all(dc.ens_seen.cpu().numpy() == n_acc)
    assert np.array_equal(dc.hitmap.cpu().numpy(), np.stack([p.values for p in posts]))          # the hit map of the same run: still exact
    assert int(dc.n_accepted.sum()) > B
    ens = ensembles.from_chains(dc)
    assert ens.thin == thin and np.all(ens.count.cpu().numpy() == n_filled) and ens.k is dc.t["ens_k"]
    assert len({float(v) for v in ens.misfit[0, :n_filled].cpu()}) > 1                           # the kept models do differ


def test_every_driver_keeps_the_same_ensemble():
    """Lock-step, persistent, cut runs and sub-blocks under the reference's schedule (burn-in reset, chains that finish)."""
    from test_unit_posteriors_gpu import _driver_runs
    runs = _driver_runs(dict(hitmap=True, ensemble=dict(n_keep=32, thin=5)))
    ref = runs[0]
    assert int((ref.status == 1).sum()) > 0 and int((ref.burned_in_iteration > 0).sum()) > 0
    k = ref.ens_k
    filled = k > 0
    for other in runs[1:]:
        for n in ("k", "sigma", "k_hist", "hitmap", "burned_in_iteration", "status", "ens_k", "ens_seen"):
            assert torch.equal(getattr(ref, n), getattr(other, n)), (other.run_mode, n)
        assert torch.equal(ref.ens_edges[filled], other.ens_edges[filled]) and torch.equal(ref.ens_misfit[filled], other.ens_misfit[filled])
        a, b = ref.ens_sigma[filled], other.ens_sigma[filled]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    seen = ref.ens_seen.long()
    assert torch.equal(seen, ref.k_hist.sum(dim=1).long())
    assert torch.equal(filled.sum(dim=1), torch.clamp((seen + 4) // 5, max=32))                  # min(n_keep, ceil(seen / thin)) slots
    done = ref.status == 1
    assert torch.all(seen[done] > 150) and torch.all(filled.sum(dim=1)[done] >= 31)             # the samples since burn-in: 5 x 30 and more
    # host replay of 24 of the chains, step by step, with the schedule's reset and stop
    B, n_it = 24, 400
    d, s, dc = _chains(B, 31, exact=True, reference_schedule=True, burn_in_min_iterations=60, n_value_bins=21,
                       options=dict(n_markov_chains=150), hitmap=True, ensemble=dict(n_keep=32, thin=5))
    rng = np.random.default_rng(4)
    dc.data.copy_(torch.as_tensor((np.tile(d["data"], (300, 1)) * rng.uniform(0.7, 1.4, (300, 1)))[:B]))
    dc._initialize()
    posts = _host_posteriors(dc)
    done, seen_bi = np.zeros(B, dtype=bool), np.full(B, -1)
    for it in range(n_it):
        dc.step()
        kk, e, sg, misfit = _states(dc)
        bi, status = dc.burned_in_iteration.cpu().numpy(), dc.status.cpu().numpy()
        for b in range(B):
            if done[b]:
                continue
            if bi[b] >= 0 and seen_bi[b] < 0:                     # burned in at this very iteration: the posteriors start over with it
                posts[b].reset()
                seen_bi[b] = bi[b]
            posts[b].update(e[b, : kk[b] - 1], sg[b, : kk[b]], misfit=misfit[b])
            done[b] = status[b] != 0
    assert done.any() and (seen_bi > 0).any()
    _compare_with_replay(dc, posts)
    assert torch.equal(dc.ens_k, ref.ens_k[:B]) and torch.equal(dc.ens_seen, ref.ens_seen[:B])     # (the same chains: keyed by row)


def test_rebin_closes_the_loop_with_the_samplers_own_posteriors():
    from test_unit_posteriors_gpu import FIRST, UNIT_KW, UNITS
    B, n_acc = 24, 150
    _, _, dc = _chains(B, 11, exact=True, ensemble=dict(n_keep=160, thin=1), **UNIT_KW)
    dc.run(50, accumulate=False)
    dc.run(n_acc)
    ens = ensembles.from_chains(dc)
    assert torch.all(ens.count == n_acc)
    axis = (dc.n_depth_bins, dc.depth_bin_width)
    out = ensembles.rebin(ens, dc.n_value_bins, dc.value_half_width, axis, units=UNITS, unit_kinds=("arithmetic", "harmonic"), **FIRST)
    for n in ("hitmap", "unit_hist", "first_hist", "first_none"):
        assert out[n].dtype == torch.int32 and torch.equal(out[n], getattr(dc, n)), n             # as integers, in every cell
    assert int(out["hitmap"].sum()) == B * n_acc * dc.n_depth_bins
    kh = torch.stack([torch.bincount(ens.k[b].long(), minlength=dc.K + 1)[: dc.K + 1] for b in range(B)])
    kh[:, 0] = 0                                                  # (k == 0 marks the empty slots)
    assert torch.equal(kh, dc.k_hist.long())
    # the outputs are what the sibling modules take
    from geobipy_amd import hitmap, unit_posteriors
    prod = hitmap.products(out["hitmap"], ens.log_mean_prior, dc.value_half_width)
    want = hitmap.products(dc.hitmap, dc.log_mean_prior, dc.value_half_width)
    assert all(torch.equal(prod[n], want[n]) for n in ("mean", "median", "total"))
    up, uw = unit_posteriors.products(out), unit_posteriors.products(dc)
    assert set(up) == set(uw) and all(np.array_equal(up[n].cpu().numpy(), uw[n].cpu().numpy(), equal_nan=True) for n in uw)
    # a finer value axis chosen afterwards: twice the cells sum pairwise to the first
    fine = ensembles.rebin(ens, 2 * dc.n_value_bins, dc.value_half_width, axis, units=UNITS, **FIRST)
    assert fine["hitmap"].shape == (B, 2 * dc.n_value_bins, dc.n_depth_bins)
    assert torch.equal(fine["hitmap"].view(B, dc.n_value_bins, 2, -1).sum(dim=2), out["hitmap"])
    assert torch.equal(fine["unit_hist"].view(B, 2, dc.n_value_bins, 2, -1).sum(dim=3), out["unit_hist"])
    assert torch.equal(fine["first_hist"], out["first_hist"]) and torch.equal(fine["first_none"], out["first_none"])
    # other thresholds, no hit map: what was not requested before the run
    other = ensembles.rebin(ens, dc.n_value_bins, dc.value_half_width, axis, first_above=(0.05, 0.2), hitmap=False)
    assert "hitmap" not in other and other["first_hist"].shape == (B, 2, dc.n_depth_bins)
    assert torch.equal((other["first_hist"].sum(dim=2) + other["first_none"]).long(), torch.full((B, 2), n_acc, device=dc.device))
    # calling again gives the same: the entry zeroes its outputs
    again = ensembles.rebin(ens, dc.n_value_bins, dc.value_half_width, axis, units=UNITS, **FIRST)
    assert all(torch.equal(again[n], out[n]) for n in ("hitmap", "unit_hist", "first_hist", "first_none"))


def _hand_made(K, z):
    """B = 3 chains of n_keep = 5 slots on the cell centres ``z``: half-space, full model, interfaces at centres, all above, all below,
    an empty slot."""
    rng = np.random.default_rng(K)
    B, n_keep = 3, 5
    k = np.zeros((B, n_keep), dtype=np.int32)
    edges, sigma = np.full((B, n_keep, K), np.inf), np.full((B, n_keep, K), np.nan)
    span = max(float(z[-1]), 1.0)

    def put(b, s, e, junk_past_k=False):
        kk = len(e) + 1
        k[b, s] = kk
        edges[b, s, : kk - 1] = e
        sigma[b, s, :kk] = rng.uniform(1e-4, 10.0, kk)
        if junk_past_k and kk < K:                                # entries past k are never read
            sigma[b, s, kk:] = -1.0
    put(0, 0, [])                                                 # a half-space
    put(0, 1, np.sort(rng.uniform(0.0, 1.2 * span, K - 1)))      # a full model, k = K
    put(0, 2, np.sort(rng.choice(z, size=min(K - 1, z.size), replace=False)))      # interfaces exactly at cell centres
    put(0, 3, np.sort(rng.uniform(-5.0, float(z[0]) - 1e-3, 3)))                  # every interface above the first centre
    put(0, 4, np.sort(rng.uniform(float(z[-1]) + 1e-3, 2.0 * span + 1.0, 3)))     # every interface below the last
    for s in range(n_keep):
        put(1, s, np.sort(rng.uniform(0.0, span, int(rng.integers(0, K)))), junk_past_k=True)
    put(2, 0, [float(z[0])]); put(2, 2, [float(z[-1])]); put(2, 4, np.sort(rng.uniform(0.0, span, 2)))       # slots 1 and 3 stay empty
    return k, edges, sigma


@pytest.mark.parametrize("K", [8, 30])
def test_raster_equals_the_numpy_rule_bit_for_bit(K):
    dev = torch.device("cuda", torch.cuda.current_device())
    for n_depth in (1, 37, 64, 65, 257):
        depth_edges = np.cumsum(np.r_[0.0, np.random.default_rng(n_depth).uniform(0.2, 1.5, n_depth)])
        z = ensembles.centres(depth_edges)
        k, edges, sigma = _hand_made(K, z)
        ens = ensembles.Ensemble(*(torch.as_tensor(a).to(dev) for a in (k, edges, sigma, np.zeros(k.shape))), (torch.as_tensor(k) > 0).sum(dim=1),
                                 1, torch.zeros(3, dtype=torch.float64, device=dev))
        for slots in (None, [4, 0, 0, 2, 1, 3, 3], [1]):
            got = ensembles.realisations(ens, depth_edges, slots=slots, log10=False).cpu().numpy()
            want = ensembles.realisations_reference(k, edges, sigma, depth_edges, slots=slots)
            assert got.shape == want.shape == (3, 5 if slots is None else len(slots), n_depth)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (n_depth, slots)
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64)), (n_depth, slots)       # a pure gather: the stored bits
        full = ensembles.realisations(ens, depth_edges, log10=False).cpu().numpy()
        assert np.all(full[0, 0] == sigma[0, 0, 0])                                   # the half-space
        assert np.all(full[0, 3] == sigma[0, 3, 3]) and np.all(full[0, 4] == sigma[0, 4, 0])      # all above: the last layer; all below: the first
        assert np.isnan(full[2, 1]).all() and np.isnan(full[2, 3]).all()              # the empty slots
        assert full[2, 0, 0] == sigma[2, 0, 1] and full[2, 2, -1] == sigma[2, 2, 1]   # an interface AT a centre: the layer below
        lg = ensembles.realisations(ens, depth_edges).cpu().numpy()
        assert np.array_equal(lg, np.log10(full), equal_nan=True) or np.allclose(lg, np.log10(full), rtol=1e-15, atol=0, equal_nan=True)


def test_a_restart_zeroes_the_ensemble():
    """infer()'s restart of stuck chains (_restart_stuck_chains) starts the ensemble over like the hit map."""
    r = np.load(os.path.join(GOLDEN, "mcmc_reset.npz"))
    window, reset_limit, n_mc = (int(x) for x in r["stuck1_meta"][:3])
    s0 = float(np.sqrt(np.prod(r["stuck1_limits"])))
    B = 8
    _, _, dc = _chains(B, 5, exact=True, reference_schedule=True, hitmap=True, ensemble=dict(n_keep=16, thin=2),
                       options=dict(n_markov_chains=n_mc, update_plot_every=window, reset_limit=reset_limit,
                                    parameter_limits=[s0 * (1.0 - 1e-9), s0 * (1.0 + 1e-9)]))
    dc.run(window - 1)
    assert int(dc.ens_seen.sum()) == B * (window - 1) and int((dc.ens_k > 0).sum()) == B * min(16, -(-(window - 1) // 2))
    snap = dc.t["n_accepted"].clone()
    dc.run(1)                                                     # the update that closes the window (infer() does the same)
    dc._restart_stuck_chains(dc.t["status"] == 0, snap, reset_limit)
    assert torch.all(dc.n_resets == 1) and torch.all(dc.iteration0 == window)
    for n in ("ens_k", "ens_seen", "hitmap", "hit_dwell"):
        assert int(dc.t[n].abs().sum()) == 0, n
    dc.run(5)                                                     # ... and it fills again from the restart
    assert torch.all(dc.ens_seen == 5) and torch.equal((dc.ens_k > 0).sum(dim=1), torch.full((B,), 3, device=dc.device))
    assert torch.all(dc.ens_k[:, :3] == 1) and torch.all(torch.isposinf(dc.ens_edges[:, :3])) and torch.all(dc.ens_k[:, 3:] == 0)


def test_sharding_does_not_change_the_ensemble():
    B, half = 64, 32
    kw = dict(hitmap=True, ensemble=dict(n_keep=24, thin=4))
    _, _, whole = _chains(B, 9, first_chain=1000, **kw)
    whole.run(120)
    for first in (0, half):
        _, _, part = _chains(half, 9, first_chain=1000 + first, **kw)
        part.run(120)
        for n in ("k", "sigma", "k_hist", "hitmap", "ens_k", "ens_edges", "ens_misfit", "ens_seen"):
            assert torch.equal(getattr(whole, n)[first:first + half], getattr(part, n)), (first, n)
        a, b = whole.ens_sigma[first:first + half], part.ens_sigma
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    assert int(whole.n_accepted.sum()) > B and torch.all(whole.ens_seen == 120) and torch.all((whole.ens_k > 0).sum(dim=1) == 24)
    assert len(torch.unique(whole.ens_k[:, 23])) > 1


def test_the_ensemble_does_not_perturb_the_chains():
    """Feature off: the chains and hit maps of a run without the ensemble equal those of the same seeds with it, in both drivers;
    ensemble, units and data posteriors together give what each gives alone."""
    from test_unit_posteriors_gpu import UNIT_KW
    state = ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "n_accepted", "k_hist", "edge_hist", "hitmap",
             "best_posterior", "best_sigma", "log_ratio")
    E = dict(n_keep=48, thin=3)
    for mode in (1, 2):
        runs = []
        for kw in (dict(hitmap=True), dict(hitmap=True, ensemble=E), dict(UNIT_KW), dict(hitmap=True, data_posteriors=True),
                   dict(UNIT_KW, data_posteriors=True, ensemble=E)):
            _, _, dc = _chains(96, 21, **kw)
            dc.run_mode = mode
            dc.run(50, accumulate=False)
            dc.run(150)
            runs.append(dc)
        off, on, units, data, allthree = runs
        assert all(off.t[n] is None for n in ENS) and off._o.n_ensemble == 0 and off._o.ensemble_thin == 0 and units.t["ens_k"] is None
        for other in (on, allthree):
            for n in state:
                assert torch.equal(getattr(off, n), getattr(other, n)), (mode, n)
        assert torch.all(on.ens_seen == 150) and torch.all((on.ens_k > 0).sum(dim=1) == 48)
        for n in ("ens_k", "ens_edges", "ens_misfit", "ens_seen"):
            assert torch.equal(getattr(on, n), getattr(allthree, n)), (mode, n)
        assert torch.equal(torch.nan_to_num(on.ens_sigma, nan=-1.0), torch.nan_to_num(allthree.ens_sigma, nan=-1.0))
        for n in ("unit_hist", "first_hist", "first_none"):
            assert torch.equal(getattr(units, n), getattr(allthree, n)), (mode, n)
        for n in ("data_hist", "misfit_hist"):
            assert torch.equal(getattr(data, n), getattr(allthree, n)), (mode, n)


def test_ensemble_arguments_are_checked_before_any_launch():
    from geobipy_amd import _lib
    with pytest.raises(ValueError, match="hitmap"):
        _chains(4, 1, ensemble=dict(n_keep=8, thin=1))           # no hit map
    with pytest.raises(ValueError, match="thin"):
        _chains(4, 1, hitmap=True, ensemble=8)                    # no schedule: thin is required
    for bad in (0, 4097, dict(n_keep=8, thin=0), dict(n_keep=8, thin=1, ring=True)):
        with pytest.raises(ValueError):
            _chains(4, 1, hitmap=True, ensemble=bad)
    _, _, sched = _chains(4, 1, hitmap=True, reference_schedule=True, ensemble=16, options=dict(n_markov_chains=100))
    assert sched.n_ensemble == 16 and sched.ensemble_thin == 7   # ceil(n_markov_chains / n_keep)
    _, _, dc = _chains(4, 1, hitmap=True, ensemble=dict(n_keep=8, thin=2))
    lib = _lib.load()
    run = lambda o, c, mode=1: lib.gbp_rj_run_mode(dc._h.ptr, o, c, 0, 1, 1, mode, dc._stream())      # noqa: E731
    for mode in (1, 2, 4):
        for field, value, word in (("n_ensemble", 0, b"n_ensemble"), ("n_ensemble", -1, b"n_ensemble"), ("n_ensemble", 4097, b"n_ensemble"),
                                   ("ensemble_thin", 0, b"ensemble_thin"), ("ensemble_thin", -3, b"ensemble_thin")):
            o = _lib.RjOptions.from_buffer_copy(dc._o)
            setattr(o, field, value)
            assert run(o, dc._c, mode) != 0, (mode, field, value)
            assert word in lib.gbp_last_error(), (mode, field, value)
        c = _lib.RjChains.from_buffer_copy(dc._c)
        c.hitmap = None
        assert run(dc._o, c, mode) != 0 and b"hit map" in lib.gbp_last_error()       # arrays without a hit map
        for name in ENS:                                          # one array without the others
            c = _lib.RjChains.from_buffer_copy(dc._c)
            setattr(c, name, None)
            assert run(dc._o, c, mode) != 0 and name.encode() in lib.gbp_last_error(), (mode, name)
    assert lib.gbp_rj_flush_posteriors(dc._o, c, dc._stream()) != 0
    assert lib.gbp_rj_run(dc._h.ptr, o, dc._c, 0, 1, 1, dc._stream()) != 0
    # the two entries on a finished ensemble
    k, e, s, lmp = dc.t["ens_k"], dc.t["ens_edges"], dc.t["ens_sigma"], dc.t["log_mean_prior"]
    K, st = dc.K, dc._stream()
    z = torch.linspace(0.5, 9.5, 10, dtype=torch.float64, device=dc.device)
    slots = torch.zeros(2, dtype=torch.int32, device=dc.device)
    out = torch.full((4, 2, 10), 7.0, dtype=torch.float64, device=dc.device)
    raster = lambda B=4, ne=8, K_=K, k_=k, R=2, nz=10, z_=z: lib.gbp_ensemble_raster(      # noqa: E731
        B, ne, K_, None if k_ is None else k_.data_ptr(), e.data_ptr(), s.data_ptr(), R, slots.data_ptr(), nz, None if z_ is None else z_.data_ptr(),
        out.data_ptr(), st)
    for kw in (dict(B=-1), dict(ne=0), dict(ne=4097), dict(K_=65), dict(K_=0), dict(R=0), dict(nz=0), dict(k_=None), dict(z_=None)):
        assert raster(**kw) != 0 and b"gbp_ensemble_raster" in lib.gbp_last_error(), kw
    assert raster(B=0, k_=None) == 0                             # an empty block: OK without a launch
    hm = torch.full((4, 6, 10), 7, dtype=torch.int32, device=dc.device)
    import ctypes
    th, di = (ctypes.c_double * 4)(0.1, 1.0, 1.0, 1.0), (ctypes.c_int32 * 4)(1, 1, 1, 1)
    fh, fn = torch.full((4, 1, 10), 7, dtype=torch.int32, device=dc.device), torch.full((4, 1), 7, dtype=torch.int32, device=dc.device)
    rebin = lambda B=4, ne=8, K_=K, nv=6, hw=2.0, nd=10, w=1.0, hm_=hm, M=0, kinds=0, T=1, th_=th, fh_=fh: lib.gbp_ensemble_rebin(      # noqa: E731
        B, ne, K_, k.data_ptr(), e.data_ptr(), s.data_ptr(), lmp.data_ptr(), nv, hw, nd, w, None if hm_ is None else hm_.data_ptr(), M, kinds, None, None,
        T, th_, di, None if fh_ is None else fh_.data_ptr(), fn.data_ptr(), st)
    for kw in (dict(B=-1), dict(ne=0), dict(ne=4097), dict(K_=65), dict(nv=0), dict(hw=0.0), dict(hw=float("nan")), dict(nd=0), dict(w=0.0),
               dict(w=float("inf")), dict(M=17), dict(M=2, kinds=0), dict(M=2, kinds=3), dict(T=5), dict(T=-1), dict(fh_=None), dict(hm_=None, T=0),
               dict(th_=(ctypes.c_double * 4)(-0.1, 1.0, 1.0, 1.0))):
        assert rebin(**kw) != 0 and b"gbp_ensemble_rebin" in lib.gbp_last_error(), kw
    assert rebin(B=0) == 0
    torch.cuda.synchronize()
    assert int(dc.k_hist.sum()) == 0 and int(dc.t["ens_seen"].sum()) == 0 and int(dc.t["ens_k"].sum()) == 0      # nothing ran
    assert torch.all(out == 7.0) and torch.all(hm == 7) and torch.all(fh == 7) and torch.all(fn == 7)          # ... and nothing was written
    with pytest.raises(ValueError):
        ensembles.realisations(ensembles.from_chains(dc), [0.0, 1.0], slots=[8])
    with pytest.raises(ValueError, match="ensemble"):
        ensembles.from_chains(_chains(2, 1, hitmap=True)[2])


def test_time_domain_chains_keep_an_ensemble():
    from geobipy_amd.tdem import TdemDeviceChains
    from test_tdem_sampler import OFFSET, _survey
    B, n_acc = 4, 120
    s, h, data, scale, opts, groups = _survey(B, seed=3)          # the golden SkyTEM low-moment system
    dc = TdemDeviceChains(s, h, data, OFFSET, seed=77, hitmap=True, ensemble=dict(n_keep=32, thin=4), **opts)
    dc.run(100, accumulate=False)
    assert int(dc.ens_seen.sum()) == 0
    posts = _host_posteriors(dc)
    for _ in range(n_acc):
        dc.step()
        k, e, sg, misfit = _states(dc)
        for b in range(B):
            posts[b].update(e[b, : k[b] - 1], sg[b, : k[b]], misfit=misfit[b])
    assert int(dc.n_accepted.sum()) > 0
    counts = _compare_with_replay(dc, posts)
    assert np.all(counts == 30) and torch.all(dc.ens_seen == n_acc)
    z = ensembles.realisations(ensembles.from_chains(dc), np.linspace(0.0, 100.0, 41), slots=[0, 29, 31])
    assert z.shape == (B, 3, 40) and not torch.isnan(z[:, :2]).any() and torch.isnan(z[:, 2]).all()


def test_replicates_concatenate_the_ensembles():
    from geobipy_amd import replicates
    S, C, nk = 6, 2, 12
    _, _, dc = _chains(S * C, 13, hitmap=True, ensemble=dict(n_keep=nk, thin=5))
    dc.run(40, accumulate=False)
    dc.run(80)
    pooled = replicates.Pooled(dc, C)
    ens = ensembles.from_chains(pooled)
    assert ens.k.shape == (S, C * nk) and ens.edges.shape == (S, C * nk, dc.K) and ens.misfit.shape == (S, C * nk)
    for n, a in (("ens_k", ens.k), ("ens_edges", ens.edges), ("ens_misfit", ens.misfit)):       # (no schedule: every chain is used)
        assert torch.equal(a, dc.t[n].view((S, C * nk) + tuple(dc.t[n].shape[2:]))), n
    assert torch.equal(torch.nan_to_num(ens.sigma, nan=-1.0), torch.nan_to_num(dc.t["ens_sigma"].view(S, C * nk, dc.K), nan=-1.0))
    assert torch.all(ens.count == C * nk) and torch.all(pooled.ens_seen == C * 80) and ens.thin == 5
    # chains that are not used leave empty slots
    t = {n: v for n, v in dc.t.items()}
    t["status"] = torch.zeros(S * C, dtype=torch.int32, device=dc.device)
    t["status"][1] = 2; t["status"][4] = 2; t["status"][5] = 2                          # replicate 1 of sounding 0, both of sounding 2
    part = replicates.Pooled(t, C, reference_schedule=True)
    k = part.ens_k.view(S, C, nk)
    assert torch.all(k[0, 0] > 0) and torch.all(k[0, 1] == 0) and torch.all(k[2] == 0) and torch.all(k[1] > 0) and torch.all(k[3:] > 0)
    assert torch.equal(part.ens_edges, ens.edges)                # (the rows stay where they are: k == 0 says "empty")
    assert int(part.ens_seen[0]) == 80 and int(part.ens_seen[2]) == 0 and int(part.ens_seen[1]) == 160


def test_survey_summaries_carry_the_ensemble(tmp_path):
    """survey.infer(ensemble=16): the kept models join the per-sounding summaries and equal ensembles.from_chains of a DeviceChains run
    of the same seeds; the command line's --ensemble writes the five arrays into the summary files."""
    from geobipy_amd import survey
    from geobipy_amd.__main__ import main
    from geobipy_amd.rjmcmc_gpu import DeviceChains
    from geobipy_amd.survey import FdemData, read_options
    options = os.path.join(GOLDEN, "resolve_options_small")
    timings = {}
    res = survey.infer(options, exact_jacobian=True, ensemble=16, timings=timings)
    assert "ensemble" in timings
    S = res["status"].size
    o = read_options(options)
    K, thin = int(o["maximum_number_of_layers"]), -(-int(o["n_markov_chains"]) // 16)
    assert res["ensemble_k"].shape == (S, 16) and res["ensemble_k"].dtype == np.int32 and res["ensemble_misfit"].shape == (S, 16)
    assert res["ensemble_edges"].shape == (S, 16, K) and res["ensemble_sigma"].shape == (S, 16, K) and np.all(res["ensemble_thin"] == thin)
    plain = survey.infer(options, exact_jacobian=True)
    for n in ("status", "n_layers", "misfit", "mean_log10_conductivity", "best_posterior", "layer_count_posterior"):
        assert np.array_equal(res[n], plain[n], equal_nan=True), n       # keeping them changes no chain
    assert not any(n.startswith("ensemble_") for n in plain)
    ds = FdemData.read_csv(o["data_filename"], o["system_filename"])
    keys = ("n_markov_chains", "solve_gradient", "maximum_number_of_layers", "minimum_depth", "maximum_depth", "minimum_thickness",
            "initial_relative_error", "minimum_relative_error", "maximum_relative_error", "initial_additive_error", "minimum_additive_error",
            "maximum_additive_error", "relative_error_proposal_variance", "additive_error_proposal_variance", "probability_of_birth",
            "probability_of_death", "probability_of_perturb", "probability_of_no_change", "factor", "gradient_standard_deviation",
            "covariance_scaling", "parameter_limits", "update_plot_every", "reset_limit", "solve_parameter", "solve_relative_error",
            "solve_additive_error")
    dc = DeviceChains(ds.system, ds.z, ds.data, seed=o.get("seed", 0), exact_jacobian=True, hitmap=True, first_chain=0, reference_schedule=True,
                      ensemble=16, **{k: o[k] for k in keys if o.get(k) is not None})
    dc.infer()
    assert np.array_equal(dc.status.cpu().numpy(), res["status"])
    ens = ensembles.from_chains(dc)
    assert ens.thin == thin
    done = res["status"] == 1
    total = res["layer_count_posterior"].sum(axis=1)             # the samples every chain accumulated
    assert done.any() and np.array_equal((res["ensemble_k"] > 0).sum(axis=1), np.minimum(16, -(-total // thin)))
    assert np.array_equal(ens.count.cpu().numpy(), (res["ensemble_k"] > 0).sum(axis=1))
    for n, v in (("ensemble_k", ens.k), ("ensemble_edges", ens.edges), ("ensemble_sigma", ens.sigma), ("ensemble_misfit", ens.misfit)):
        assert np.array_equal(res[n], v.cpu().numpy(), equal_nan=True), n
    # the command line
    out = tmp_path / "cli"
    out.mkdir()
    assert main([options, str(out), "--exact-jacobian", "--no-containers", "--ensemble", "8"]) == 0
    ln = np.unique(res["line"])[0]
    line = np.load(str(out / "{}.npz".format(ln)))
    n_line = int((res["line"] == ln).sum())
    for n, shape in (("ensemble_k", (n_line, 8)), ("ensemble_edges", (n_line, 8, K)), ("ensemble_sigma", (n_line, 8, K)),
                     ("ensemble_misfit", (n_line, 8)), ("ensemble_thin", (n_line,))):
        assert n in line.files and line[n].shape == shape, n
    assert np.all(line["ensemble_thin"] == -(-int(o["n_markov_chains"]) // 8))
