"""Sections of sampled models on the device (csrc/gbp_ensemble_families.h k_layered_cross_distance<linear / log>, csrc/gbp_section.h
k_section_viterbi / k_section_marginals; geobipy_amd.sections).

The cross distance is held to the existing distance kernel with ``==`` on the bits (the off-diagonal block of ``families.distance`` on
the stacked slots), and to the rule in long double with the a-priori bound test_families_gpu.py derives for the same sum.  With
U = 2^-52, K the layer capacity, D2 the rule's squared distance and a_max the largest |log10 sigma|:
    stored values (log10 = 0)   |dD2| <= (2 K + 16) U D2            (+ 8 U D2 for the log measure: ln of every segment)
    log10 taken on the device   |dD2| <= the same + 16 U a_max D + (8 U a_max)^2
and for D = sqrt(D2) with e the bound of D2: |dD| <= min(e / D, sqrt(e)) + 2 U D.  Every case prints used / bound.

The chain is held to ``sections.track_reference``: the path and its score with ``==``, the marginals within max(16 e, 16 * 2^-52) of the
long-double rule, e the fp64 rule's own distance from it (the bound of test_horizons_gpu.py)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, ensembles, families, sections
from test_families_gpu import _hand_made, _to_device
from test_rjmcmc_gpu import GOLDEN, _chains
from test_sections import Z1_LINE, check_planted_line, planted_line

U = 2.0 ** -52


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for n, v in d.items()}


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- the cross distance -------------------------------------------------------------------------------------------------------------

def _pair_of_soundings(n, K):
    """The two hand-made soundings of test_families_gpu.py (copies, an empty slot, rows -1 and past the end, interfaces on the window's
    ends); where there is room, slot 4 of sounding 1 becomes a copy of slot 0 of sounding 0: one model under two soundings."""
    k, edges, sigma, rows = _hand_made(n, K, 100 * n + K)
    if k.shape[1] > 5:
        k[1, 4], edges[1, 4], sigma[1, 4] = k[0, 0], edges[0, 0], sigma[0, 0]
    return k, edges, sigma, rows


def _stacked_block(k, edges, sigma, rows, s, p, z0, z1, **kw):
    """The block [:n, n:] of families.distance on the slots of soundings s and p stacked into one sounding."""
    ns, n = k.shape[1], rows.shape[1]
    valid = lambda r: np.where((r >= 0) & (r < ns), r, -1)                     # noqa: E731  (a row past the end must not name the other's slot)
    both = np.concatenate([valid(rows[s]), np.where(valid(rows[p]) >= 0, valid(rows[p]) + ns, -1)]).astype(np.int32)
    ens = _to_device(np.concatenate([k[s], k[p]])[None], np.concatenate([edges[s], edges[p]])[None], np.concatenate([sigma[s], sigma[p]])[None])
    return families.distance(ens, torch.as_tensor(both[None]).to(_dev()), z0, z1, **kw)[0, :n, n:]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("K", [1, 2, 7, 64])
def test_cross_distance_equals_the_existing_kernel(n, K):
    z0, z1 = 5.0, 200.0
    k, edges, sigma, rows = _pair_of_soundings(n, K)
    for measure in ("linear", "log"):
        for log10 in (True, False):
            sg = sigma if log10 else np.where(sigma > 0, np.log10(np.where(sigma > 0, sigma, 1.0)), sigma)
            ens, rows_d = _to_device(k, edges, sg), torch.as_tensor(rows).to(_dev())
            for squared in (True, False):
                kw = dict(measure=measure, squared=squared, log10=log10)
                got = sections.cross_distance(ens, rows_d, np.array([1, 0], dtype=np.int32), z0, z1, **kw)
                again = sections.cross_distance(ens, rows_d, torch.tensor([1, 0], dtype=torch.int32), z0, z1, **kw)
                assert got.shape == (2, n, n) and got.dtype == torch.float64 and torch.equal(_bits(got), _bits(again))      # a second call, bit for bit
                for s, p in ((0, 1), (1, 0)):
                    want = _stacked_block(k, edges, sg, rows, s, p, z0, z1, **kw)
                    assert torch.equal(_bits(got[s]), _bits(want)), (measure, log10, squared, s)      # values and NaN patterns alike
                absent = [np.array([not (0 <= r < k.shape[1]) or k[b, min(max(r, 0), k.shape[1] - 1)] <= 0 for r in rows[b]]) for b in range(2)]
                g0 = got[0].cpu().numpy()
                assert np.array_equal(np.isnan(g0), absent[0][:, None] | absent[1][None, :])
                if k.shape[1] > 5:                                             # one model under both soundings: 0.0 by arithmetic
                    same = np.isin(rows[0], (0, 1))[:, None] & (rows[1] == 4)[None, :]
                    assert np.all(g0[same] == 0.0)
                alone = sections.cross_distance(ens, rows_d, [1, -1], z0, z1, **kw)
                assert torch.equal(_bits(alone[0]), _bits(got[0])) and bool(torch.isnan(alone[1]).all())
                outside = sections.cross_distance(ens, rows_d, [2, -7], z0, z1, **kw)
                assert bool(torch.isnan(outside).all())
    blocks = sections.cross_distance(ens, rows_d, [1, 0], z0, z1, block=1)      # a block brings its partner along: the same bits
    assert torch.equal(_bits(blocks), _bits(sections.cross_distance(ens, rows_d, [1, 0], z0, z1)))


@pytest.mark.parametrize("n,K", [(1, 1), (17, 2), (17, 64), (33, 7)])
def test_cross_distance_against_the_long_double_rule(n, K):
    z0, z1 = 5.0, 200.0
    k, edges, sigma, rows = _pair_of_soundings(n, K)
    partner = np.array([1, 0], dtype=np.int32)
    for measure in ("linear", "log"):
        for stored in (True, False):
            sg = np.where(sigma > 0, np.log10(np.where(sigma > 0, sigma, 1.0)), sigma) if stored else sigma
            ens, rows_d = _to_device(k, edges, sg), torch.as_tensor(rows).to(_dev())
            got2 = sections.cross_distance(ens, rows_d, partner, z0, z1, measure=measure, squared=True, log10=not stored).cpu().numpy()
            got1 = sections.cross_distance(ens, rows_d, partner, z0, z1, measure=measure, squared=False, log10=not stored).cpu().numpy()
            want2 = sections.cross_distance_reference(k, edges, sg, rows, partner, z0, z1, measure=measure, dtype=np.longdouble, stored=stored)
            want1 = np.sqrt(want2)
            worst2 = worst1 = 0.0
            for b in range(2):
                ok = ~np.isnan(want2[b])
                assert np.array_equal(np.isnan(got2[b]), ~ok) and np.array_equal(np.isnan(got1[b]), ~ok)
                if not ok.any():
                    continue
                a_max = 0.0 if stored else max(float(np.nanmax(np.abs(np.log10(np.where(sigma[c] > 0, sigma[c], np.nan))))) for c in range(2))
                w2, w1 = want2[b][ok], want1[b][ok]
                e2 = (2 * K + 16 + (8 if measure == "log" else 0)) * U * w2 + (16 * U * a_max * w1 + (8 * U * a_max) ** 2 if not stored else 0.0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    e1 = np.minimum(np.where(w1 > 0, e2 / w1, np.inf), np.sqrt(e2)) + 2 * U * w1
                d2, d1 = np.abs(got2[b][ok].astype(np.longdouble) - w2), np.abs(got1[b][ok].astype(np.longdouble) - w1)
                assert np.all(d2 <= e2), (measure, stored, b, "D2", float(np.max(d2 - e2)))
                assert np.all(d1 <= e1), (measure, stored, b, "D", float(np.max(d1 - e1)))
                live = e2 > 0
                if live.any():
                    worst2, worst1 = max(worst2, float(np.max(d2[live] / e2[live]))), max(worst1, float(np.max(d1[live] / e1[live])))
            print("n=%d K=%d %s %s used/bound: D2 %.3f D %.3f" % (n, K, measure, "stored" if stored else "log10", worst2, worst1))


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def _chain_case(n, lengths, seed, exact=False):
    """Scores, steps and squared distances of the sequences, made once in numpy for both sides: ragged n_used with 1 and n among them,
    NaN everywhere outside the prefixes i < m_r, j < m_{r+1} and in the entry of every sequence's last sounding."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n_used = rng.integers(1, n + 1, total).astype(np.int32)
    n_used[-1], n_used[-2] = 1, n                                              # the longest sequence ends n -> 1
    n_used[ptr[-2]] = max(1, n // 2)
    if exact:
        score, g, d2 = rng.integers(0, 3, (total, n)).astype(np.float64), np.ones(total), rng.integers(0, 17, (total, n, n)) / 8.0
    else:
        score, g, d2 = rng.normal(0.0, 1.5, (total, n)), rng.uniform(0.5, 4.0, total), rng.uniform(0.0, 1.5, (total, n, n))
    last = np.zeros(total, dtype=bool)
    last[ptr[1:] - 1] = True
    for r in range(total):
        if last[r]:
            d2[r] = np.nan
            continue
        d2[r, n_used[r]:, :] = np.nan
        d2[r, :, n_used[r + 1]:] = np.nan
    return ptr, score, g, d2, n_used


def _device_track(ptr, score, g, d2, n_used, marginals=True):
    dev = _dev()
    out = sections.track(torch.as_tensor(d2).to(dev), g, ptr, n_used, score=None if score is None else torch.as_tensor(score).to(dev), marginals=marginals)
    torch.cuda.synchronize()
    return _numpy(out)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1024])
def test_chain_against_the_rule(n):
    lengths = (1, 2, 3) if n == 1024 else (1, 2, 7)
    ptr, score, g, d2, n_used = _chain_case(n, lengths, 500 + n)
    got = _device_track(ptr, score, g, d2, n_used)
    ref = sections.track_reference(ptr, score, g, d2, n_used)
    assert got["state"].dtype == np.int32 and np.array_equal(got["state"], ref["state"])
    assert np.array_equal(got["log_score"], ref["log_score"])
    assert np.all(got["state"] < n_used) and np.all(got["state"] >= 0)
    ld = sections.track_reference(ptr, score, g, d2, n_used, dtype=np.longdouble)
    assert np.array_equal(ld["state"], ref["state"])
    m_ld = ld["marginal"]
    assert np.all(np.isfinite(m_ld.astype(np.float64)))                       # the inputs stay clear of underflow
    e = float(np.abs(ref["marginal"] - m_ld).max())
    bound = max(16.0 * e, 16.0 * U)
    dist = float(np.abs(got["marginal"] - m_ld).max())
    rows = float(np.abs(got["marginal"].sum(axis=1) - 1.0).max())
    lp_bound = np.array([16.0 * U * (m + np.abs(np.log(ld["scale"][a:a + m].astype(np.float64))).sum()) for a, m in zip(ptr[:-1], lengths)])
    lp_dist = np.abs(got["log_partition"] - ld["log_partition"]).astype(np.float64)
    print("n=%d: e=%.3g bound=%.3g device distance=%.3g rows=%.3g log_partition distance=%.3g (bound %.3g)"
          % (n, e, bound, dist, rows, lp_dist.max(), lp_bound.min()))
    assert got["marginal"].shape == (int(ptr[-1]), n)
    assert dist <= bound
    assert rows <= bound
    for r in range(int(ptr[-1])):
        assert np.all(got["marginal"][r, n_used[r]:] == 0.0)
    assert np.all(lp_dist <= lp_bound)
    assert float(np.abs(got["scale"] / ld["scale"].astype(np.float64) - 1.0).max()) <= 64.0 * U
    w = np.exp(score[0, :n_used[0]])                                           # the sequence of one sounding: the normalised w
    assert float(np.abs(got["marginal"][0, :n_used[0]] - w / w.sum()).max()) <= 16.0 * U


@pytest.mark.parametrize("n", [3, 70, 128, 300, 600])
def test_exact_ties_follow_the_tie_order(n):
    """d2 in multiples of 1/8, integer scores and g = 1: every operation is exact, many paths score the same, and the device picks the
    one the rule picks -- across the lane groups that share the i range (n <= 128) as within one lane's loop."""
    ptr, score, g, d2, n_used = _chain_case(n, (1, 2, 9), 9 + n, exact=True)
    got = _device_track(ptr, score, g, d2, n_used, marginals=False)
    ref = sections.track_reference(ptr, score, g, d2, n_used, marginals=False)
    assert np.array_equal(got["state"], ref["state"]) and np.array_equal(got["log_score"], ref["log_score"])
    flat = _device_track(ptr, None, g, np.where(np.isnan(d2), d2, 0.0), n_used, marginals=False)
    assert not flat["state"].any() and not flat["log_score"].any()             # all ties: the lowest state everywhere


def test_degenerate_launches():
    dev, lib = _dev(), _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    # every sequence holds one sounding
    ptr, score, g, d2, n_used = _chain_case(5, (1, 1, 1, 1), 3)
    n_used[:] = [5, 1, 3, 2]
    got = _device_track(ptr, score, g, d2, n_used)
    ref = sections.track_reference(ptr, score, g, d2, n_used)
    assert np.array_equal(got["state"], ref["state"]) and np.array_equal(got["log_score"], ref["log_score"])
    assert np.allclose(got["marginal"], ref["marginal"], rtol=0, atol=16 * U) and np.allclose(got["log_partition"], ref["log_partition"], rtol=0, atol=1e-14)
    # marginals off: the Viterbi launch alone
    ptr, score, g, d2, n_used = _chain_case(65, (1, 2, 7), 4)
    quick = _device_track(ptr, score, g, d2, n_used, marginals=False)
    ref = sections.track_reference(ptr, score, g, d2, n_used, marginals=False)
    assert set(quick) == {"state", "log_score"} and np.array_equal(quick["state"], ref["state"]) and np.array_equal(quick["log_score"], ref["log_score"])
    # L == 0: nothing is launched, the outputs keep their values
    state = torch.full((4,), -7, dtype=torch.int32, device=dev)
    assert lib.gbp_section_track(0, None, 0, 5, None, None, None, None, None, state.data_ptr(), None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert bool((state == -7).all())
    none = sections.track(torch.zeros((0, 5, 5), dtype=torch.float64, device=dev), np.zeros(0), [0], np.zeros(0, dtype=np.int32))
    assert none["state"].shape == (0,) and none["log_score"].shape == (0,) and none["marginal"].shape == (0, 5)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_the_planted_line_on_the_device():
    k, edges, sigma, x, y, truth = planted_line()
    S, n = k.shape
    ens = _to_device(k, edges, sigma)
    out = sections.sections(ens, x, y, Z1_LINE)
    assert np.array_equal(out["rows"].cpu().numpy(), np.tile(np.arange(n), (S, 1))) and bool((out["n_used"] == n).all())
    partner = sections.partners(None, out["n_used"])
    d2 = sections.cross_distance(ens, out["rows"], partner, 0.0, Z1_LINE)
    host = d2.cpu().numpy()
    ref = sections.track_reference([0, S], None, sections.steps(x, y), host, np.full(S, n))
    o = _numpy(out)
    assert np.array_equal(o["state"], ref["state"]) and np.array_equal(o["log_score"], ref["log_score"])      # the rule on the device's own d2
    assert np.allclose(o["weight"], ref["marginal"], rtol=0, atol=1e-13) and abs(o["log_partition"][0] - ref["log_partition"][0]) <= 1e-10
    check_planted_line(lambda g: sections.track(d2, g, [0, S], np.full(S, n), marginals=False)["state"].cpu().numpy(), k, edges, sigma, x, y, truth)
    assert np.array_equal(o["slot"], o["state"]) and np.array_equal(o["section_edges"], edges[np.arange(S), o["state"]])
    assert np.all(np.abs(o["section_edges"][:, 0] - truth) <= 4.0) and np.all(o["section_k"] == 3)
    assert np.isnan(o["step_distance"][-1]) and np.all(o["step_distance"][:-1] < 0.45)     # no jump of 15 m (0.53 decades) anywhere on the path
    assert np.all(o["n_effective"] >= 1.0 - 1e-12) and np.all(o["n_effective"] <= n + 1e-9)
    assert np.array_equal(o["chosen_weight"], o["weight"][np.arange(S), o["state"]])


def test_sections_of_real_chains():
    B, nk, thin = 16, 32, 2
    _, _, dc = _chains(B, 17, exact=True, hitmap=True, ensemble=dict(n_keep=nk, thin=thin))
    dc.run(60, accumulate=False)
    dc.run(nk * thin)
    z1 = float(dc.n_depth_bins * dc.depth_bin_width)
    ens = ensembles.from_chains(dc)
    kk = ens.k.clone()
    kk[3] = 0                                                                  # a sounding without models cuts its sequence
    ens = ens._replace(k=kk)
    x, y, ptr = 20.0 * np.arange(B), np.zeros(B), np.array([0, 7, B])
    out = sections.sections(ens, x, y, z1, ptr=ptr, max_models=16)
    o = _numpy(out)
    k, edges, sigma = (a.cpu().numpy() for a in (ens.k, ens.edges, ens.sigma))
    has = np.arange(B) != 3
    assert o["n_used"][3] == 0 and np.all(o["n_used"][has] == 16) and o["rows"].shape == (B, 16)
    assert o["state"][3] == -1 and o["slot"][3] == -1 and o["section_k"][3] == 0 and np.isnan(o["section_edges"][3]).all() and np.isnan(o["weight"][3]).all()
    assert np.isnan(o["n_effective"][3]) and np.isnan(o["chosen_weight"][3])
    at = np.nonzero(has)[0]
    assert np.all(o["state"][at] >= 0) and np.all(o["state"][at] < 16) and np.array_equal(o["slot"][at], o["rows"][at, o["state"][at]])
    assert np.all(k[at, o["slot"][at]] > 0) and np.array_equal(o["section_k"][at], k[at, o["slot"][at]])      # every slot is a filled slot
    assert np.array_equal(o["section_edges"][at].view(np.int64), edges[at, o["slot"][at]].view(np.int64))      # bit copies
    assert np.array_equal(o["section_sigma"][at].view(np.int64), sigma[at, o["slot"][at]].view(np.int64))
    partner = sections.partners(ptr, o["n_used"])
    assert partner.tolist() == [1, 2, -1, -1, 5, 6, -1] + list(range(8, B)) + [-1]
    d2_dev = sections.cross_distance(ens, out["rows"], partner, 0.0, z1)
    d2 = d2_dev.cpu().numpy()
    for s in range(B):
        if partner[s] < 0:
            assert np.isnan(o["step_distance"][s])
        else:
            entry = d2[s, o["state"][s], o["state"][s + 1]]
            assert abs(o["step_distance"][s] ** 2 - entry) <= 4 * U * entry       # step_distance^2 is the d2 entry of the chosen pair
            assert o["step_distance"][s] == float(torch.sqrt(d2_dev[s, o["state"][s], o["state"][s + 1]]))
    assert np.all(o["n_effective"][at] >= 1.0 - 1e-12) and np.all(o["n_effective"][at] <= o["n_used"][at] + 1e-9)
    assert np.allclose(o["weight"][at].sum(axis=1), 1.0, rtol=0, atol=1e-12) and o["log_score"].shape == (2,) and o["log_partition"].shape == (2,)
    # the rule on the device's distances, run by run
    g = sections.steps(x, y, ptr=ptr)
    tops = []
    for a, b in ((0, 3), (4, 7), (7, B)):
        ref = sections.track_reference([0, b - a], None, g[a:b], d2[a:b], o["n_used"][a:b])
        assert np.array_equal(o["state"][a:b], ref["state"])
        tops.append(ref["log_score"][0])
    assert o["log_score"][0] == tops[0] + tops[1] and o["log_score"][1] == tops[2]      # a cut sequence: the sum over its runs
    # one run per launch: the same arrays
    small = _numpy(sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, budget_bytes=9 * 16 * 16 * 8))
    assert all(np.array_equal(small[name], o[name], equal_nan=True) for name in o)
    quick = sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, marginals=False)
    assert set(quick) == set(out) - {"weight", "chosen_weight", "n_effective", "log_partition"} and torch.equal(quick["state"], out["state"])
    with pytest.raises(ValueError, match="max_models.*budget_bytes"):
        sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, budget_bytes=8 * 16 * 16 * 8)


def test_from_survey_and_the_command_line(tmp_path):
    from geobipy_amd import survey
    res = survey.infer(os.path.join(GOLDEN, "resolve_options_small"), exact_jacobian=True, ensemble=16)
    z1 = 120.0
    direct = sections.from_survey(res, z1, z0=2.0, measure="log", tau=0.2)
    path = str(tmp_path / "survey.npz")
    res.save(path)
    loaded = sections.from_survey(path, z1, z0=2.0, measure="log", tau=0.2)
    written = sections.main([path, "--depth", "120", "--from", "2", "--measure", "log", "--tau", "0.2"])
    assert written == str(tmp_path / "survey.sections.npz")
    f, d, l = sections.load(written), _numpy(direct), _numpy(loaded)
    S = res["line"].size
    assert set(f) == set(d) == set(l) and {"line", "fiducial", "x", "y", "state", "slot", "section_edges", "weight", "log_partition"} <= set(f)
    for name in d:
        assert np.array_equal(f[name], d[name], equal_nan=True) and np.array_equal(l[name], d[name], equal_nan=True), name
    ptr = sections.line_ptr(res["line"])
    assert d["state"].shape == (S,) and d["log_score"].shape == (ptr.size - 1,) and np.array_equal(d["line"], res["line"])
    usable = (res["ensemble_k"] > 0).sum(axis=1) >= 8
    assert usable.any() and np.all(d["state"][usable] >= 0) and np.all(d["state"][~usable] == -1)
    at = np.nonzero(usable)[0]
    assert np.array_equal(d["section_edges"][at], res["ensemble_edges"][at, d["slot"][at]])
    no = sections.load(sections.main([path, "--depth", "120", "--no-marginals"]))
    assert "weight" not in no and no["state"].shape == (S,)


def test_the_c_entries_refuse_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    S, ns, K, n = 2, 6, 4, 5
    k = torch.ones((S, ns), dtype=torch.int32, device=dev)
    e = torch.full((S, ns, K), float("inf"), dtype=torch.float64, device=dev)
    s = torch.ones((S, ns, K), dtype=torch.float64, device=dev)
    rows = torch.zeros((S, n), dtype=torch.int32, device=dev)
    partner = torch.tensor([1, -1], dtype=torch.int32, device=dev)
    dist = torch.full((S, n, n), 7.0, dtype=torch.float64, device=dev)
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    cross = lambda S_=S, ns_=ns, K_=K, k_=k, e_=e, s_=s, n_=n, rows_=rows, pa=partner, z0=0.0, z1=10.0, measure=0, dist_=dist: \
        lib.gbp_ensemble_cross_distance(S_, ns_, K_, p(k_), p(e_), p(s_), n_, p(rows_), p(pa), z0, z1, measure, 1, 1, p(dist_), st)      # noqa: E731
    inf, nan = float("inf"), float("nan")
    for kw in (dict(S_=-1), dict(ns_=0), dict(K_=0), dict(K_=65), dict(n_=0), dict(n_=4097), dict(z0=-1.0), dict(z1=0.0), dict(z0=10.0), dict(z1=inf),
               dict(z0=nan), dict(z1=nan), dict(measure=2), dict(measure=-1), dict(measure=1), dict(k_=None), dict(e_=None), dict(s_=None),
               dict(rows_=None), dict(pa=None), dict(dist_=None), dict(S_=2 ** 16, n_=4096), dict(S_=2 ** 24)):
        assert cross(**kw) != 0 and b"gbp_ensemble_cross_distance" in lib.gbp_last_error(), kw
    assert cross(S_=0, k_=None) == 0                                     # an empty block: OK without a launch
    T, L = 3, 2
    ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device=dev)
    nu = torch.full((T,), n, dtype=torch.int32, device=dev)
    score, g, d2 = (torch.zeros(shape, dtype=torch.float64, device=dev) for shape in ((T, n), (T,), (T, n, n)))
    back = torch.full((T, n), 7, dtype=torch.int16, device=dev)
    state = torch.full((T,), 7, dtype=torch.int32, device=dev)
    ls, lp = (torch.full((L,), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
    mg, sc = torch.full((T, n), 7.0, dtype=torch.float64, device=dev), torch.full((T,), 7.0, dtype=torch.float64, device=dev)
    track = lambda L_=L, ptr_=ptr, T_=T, n_=n, nu_=nu, score_=score, g_=g, d2_=d2, back_=back, state_=state, ls_=ls, mg_=mg, lp_=lp, sc_=sc: \
        lib.gbp_section_track(L_, p(ptr_), T_, n_, p(nu_), p(score_), p(g_), p(d2_), p(back_), p(state_), p(ls_), p(mg_), p(lp_), p(sc_), st)      # noqa: E731
    for kw in (dict(L_=-1), dict(n_=0), dict(n_=1025), dict(T_=1), dict(T_=2 ** 62), dict(ptr_=None), dict(nu_=None), dict(score_=None), dict(g_=None),
               dict(d2_=None), dict(back_=None), dict(state_=None), dict(ls_=None), dict(mg_=None), dict(lp_=None), dict(sc_=None),
               dict(mg_=None, lp_=None), dict(lp_=None, sc_=None)):
        assert track(**kw) != 0 and b"gbp_section_track" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    assert torch.all(dist == 7.0) and torch.all(back == 7) and torch.all(state == 7) and torch.all(ls == 7.0) and torch.all(mg == 7.0)
    assert torch.all(lp == 7.0) and torch.all(sc == 7.0)                 # nothing was written
