"""Joint draws of sections on the device (csrc/gbp_section.h k_section_filter / k_section_draw; geobipy_amd.sections draw, sections(...,
draws=), draw_models, exceedance_area), held to ``sections.draw_reference``.

The filter is held within max(16 e, 16 * 2^-52) of the long-double rule, e the fp64 rule's own distance from it: the bound of
test_sections_gpu.py test_chain_against_the_rule for the same forward pass.  The draws are compared with ``==`` wherever the fp64 rule
decided every step of the walk by a margin of at least 1e-9 of the cumulative sum's total: the device's exp is not numpy's to the last
bit, so a draw nearer than that to a boundary may fall either way, and the rest of that walk differs.  n * bound <= 1e-10 is asserted,
so the threshold stands three orders above what the filter's rounding can move a cumulative sum; at most 1 % of the (realisation,
sequence) pairs of a case may be left out, and every case prints how many were.

Sums taken in another order (draw_log_score, exceedance_area) are held to the a-priori bound N * 2^-52 * sum |terms| of a sum of N
terms: (N - 1) 2^-53 sum |terms| for each of the two evaluations."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, ensembles, sections
from test_families_gpu import _to_device
from test_rjmcmc_gpu import GOLDEN, _chains
from test_section_draws import R_STAT, check_marginal_frequencies, ragged_chain
from test_sections import Z1_LINE, planted_line
from test_sections_gpu import _chain_case, _dev, _numpy

U = 2.0 ** -52
CLOSE = 1.0e-9


def _device_draw(ptr, score, g, d2, n_used, R, **kw):
    dev = _dev()
    out = sections.draw(torch.as_tensor(d2).to(dev), g, ptr, n_used, R, score=None if score is None else torch.as_tensor(score).to(dev), **kw)
    torch.cuda.synchronize()
    return _numpy(out)


def _left_out(margin, ptr):
    """bool [R, L]: the (realisation, sequence) pairs in which a step of the fp64 rule came within CLOSE of another outcome."""
    close = margin < CLOSE
    return np.stack([close[:, a:b].any(axis=1) if b > a else np.zeros(close.shape[0], dtype=bool) for a, b in zip(ptr[:-1], ptr[1:])], axis=1)


def _check_draws(got, ref, ptr, n_used, what):
    """``got`` [R, T] equals the rule's draws in every pair that is not left out; at most 1 % are; every state lies in 0 .. m - 1."""
    out = _left_out(ref["margin"], ptr)
    share = float(out.mean()) if out.size else 0.0
    print("%s: %d of %d (realisation, sequence) pairs left out; smallest margin %.3g" % (what, int(out.sum()), out.size, float(ref["margin"].min(initial=1.0))))
    assert share <= 0.01
    assert got.dtype == np.int32 and got.shape == ref["draw_state"].shape
    for l, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        keep = ~out[:, l]
        assert np.array_equal(got[keep, a:b], ref["draw_state"][keep, a:b]), (what, l)
    assert np.all(got >= 0) and np.all(got < np.asarray(n_used)[None, :])


def _check_against_the_rule(ptr, score, g, d2, n_used, R, what, **kw):
    n = d2.shape[1]
    got = _device_draw(ptr, score, g, d2, n_used, R, seed=7, **kw)
    ref = sections.draw_reference(ptr, score, g, d2, n_used, R, seed=7, **kw)
    ld = sections.draw_reference(ptr, score, g, d2, n_used, 1, seed=7, dtype=np.longdouble, **kw)["filtered"]
    assert np.all(np.isfinite(ld.astype(np.float64)))
    e = float(np.abs(ref["filtered"] - ld).max())
    bound = max(16.0 * e, 16.0 * U)
    dist = float(np.abs(got["filtered"] - ld).max())
    print("%s: filter e=%.3g bound=%.3g device distance=%.3g" % (what, e, bound, dist))
    assert got["filtered"].shape == (int(ptr[-1]), n) and dist <= bound
    assert n * bound <= 1.0e-10                                                # the close-call threshold stands well above the filter's rounding
    for r in range(int(ptr[-1])):
        assert np.all(got["filtered"][r, n_used[r]:] == 0.0)
    _check_draws(got["draw_state"], ref, ptr, n_used, what)
    return got


@pytest.mark.parametrize("n,R", [(1, 5), (2, 65), (63, 300), (64, 64), (65, 63), (257, 129), (1024, 65)])
def test_draws_against_the_rule(n, R):
    lengths = (1, 2, 3) if n == 1024 else (1, 2, 7)
    ptr, score, g, d2, n_used = _chain_case(n, lengths, 500 + n)
    _check_against_the_rule(ptr, score, g, d2, n_used, R, "n=%d R=%d" % (n, R))


def test_an_empty_sequence_and_keys_beyond_32_bits():
    ptr, score, g, d2, n_used = _chain_case(17, (1, 2, 7), 517)
    ptr = np.array([0, 1, 3, 3, 10], dtype=np.int64)                           # ptr repeated: the third sequence holds no sounding
    key = (2 ** 32 + 5 + 3 * np.arange(10) + (np.arange(10) % 3) * 2 ** 40).astype(np.int64)
    got = _check_against_the_rule(ptr, score, g, d2, n_used, 70, "empty sequence, 64-bit keys", row_key=key)
    low = _device_draw(ptr, score, g, d2, n_used, 70, seed=7, row_key=key & 0xFFFFFFFF)
    assert not np.array_equal(low["draw_state"], got["draw_state"])            # the high word of a key is used
    on_device = _device_draw(ptr, score, g, d2, n_used, 70, seed=7, row_key=torch.as_tensor(key).to(_dev()))
    assert np.array_equal(on_device["draw_state"], got["draw_state"])


def test_a_call_repeats_its_bits_and_a_draw_does_not_depend_on_their_number():
    ptr, score, g, d2, n_used = _chain_case(65, (1, 2, 7), 565)
    a, b = (_device_draw(ptr, score, g, d2, n_used, 65, seed=2 ** 40 + 9) for _ in range(2))
    assert np.array_equal(a["draw_state"], b["draw_state"]) and np.array_equal(a["filtered"].view(np.int64), b["filtered"].view(np.int64))
    one = _device_draw(ptr, score, g, d2, n_used, 1, seed=2 ** 40 + 9)
    assert np.array_equal(one["draw_state"][0], a["draw_state"][0]) and np.array_equal(one["filtered"].view(np.int64), a["filtered"].view(np.int64))
    assert not np.array_equal(_device_draw(ptr, score, g, d2, n_used, 65, seed=9)["draw_state"], a["draw_state"])      # the seed's high word is used
    none = sections.draw(torch.zeros((0, 5, 5), dtype=torch.float64, device=_dev()), np.zeros(0), [0], np.zeros(0, dtype=np.int32), 3)
    assert none["draw_state"].shape == (3, 0) and none["filtered"].shape == (0, 5)


def test_the_devices_own_draws_follow_the_smoothed_marginals():
    ptr, score, g, d2, n_used = ragged_chain(21, 6, 12)
    ld = sections.track_reference(ptr, score, g, d2, n_used, dtype=np.longdouble)
    got = _device_draw(ptr, score, g, d2, n_used, R_STAT, seed=3)
    check_marginal_frequencies(got["draw_state"], ld["marginal"].astype(np.float64), n_used, R_STAT, "device, n = 6, N = 12")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def _path_terms(state, score, g, d2, partner):
    """(sum of the terms, sum of their absolute values) of a path [S] with models everywhere: score[s, state] - g d2 along the steps."""
    s = np.arange(state.size)
    step = np.where(partner >= 0, g * d2[s, state, state[np.where(partner >= 0, partner, 0)]], 0.0)
    sc = np.zeros(state.size) if score is None else score[s, state]
    return float(sc.sum() - step.sum()), float(np.abs(sc).sum() + np.abs(step).sum())


def test_the_planted_line_with_draws():
    k, edges, sigma, x, y, truth = planted_line()
    S, n = k.shape
    R = 64
    ens = _to_device(k, edges, sigma)
    out = sections.sections(ens, x, y, Z1_LINE, draws=R, seed=5)
    plain = sections.sections(ens, x, y, Z1_LINE)
    assert set(out) == set(plain) | {"draw_state", "draw_slot", "draw_log_score"}
    for name in plain:                                                         # draws change no other output
        assert torch.equal(out[name].view(torch.int64) if out[name].dtype == torch.float64 else out[name],
                           plain[name].view(torch.int64) if plain[name].dtype == torch.float64 else plain[name]), name
    o = _numpy(out)
    assert o["draw_state"].shape == (R, S) and o["draw_state"].dtype == np.int32 and o["draw_slot"].dtype == np.int32 and o["draw_log_score"].shape == (R, 1)
    assert np.array_equal(o["draw_slot"], o["draw_state"]) and np.all(o["draw_state"] >= 0) and np.all(o["draw_state"] < n)
    partner = sections.partners(None, out["n_used"])
    d2 = sections.cross_distance(ens, out["rows"], partner, 0.0, Z1_LINE).cpu().numpy()
    g = sections.steps(x, y)
    ref = sections.draw_reference([0, S], None, g, d2, np.full(S, n), R, seed=5)      # the rule on the device's own d2; the key is the sounding's index
    _check_draws(o["draw_state"], ref, np.array([0, S]), np.full(S, n), "planted line")
    near = lambda st: (np.abs(edges[np.arange(S)[None, :], st, 0] - truth[None, :]) <= 4.0).mean(axis=1)      # noqa: E731
    share, share_ref = near(o["draw_state"]), near(ref["draw_state"])
    print("first interface within 4 m: device %.2f .. %.2f of the soundings, rule %.2f .. %.2f" % (share.min(), share.max(), share_ref.min(), share_ref.max()))
    assert np.all(share >= share_ref.min()) and share_ref.min() >= 0.5
    for r in range(R):
        total, size = _path_terms(o["draw_state"][r], None, g, d2, partner)
        assert o["draw_log_score"][r, 0] <= o["log_score"][0] + S * U * size
        assert abs(o["draw_log_score"][r, 0] - total) <= S * U * size
    # a score that all but fixes the path: realisations equal to the Viterbi path, whose draw_log_score is log_score to rounding
    score = np.zeros((S, n))
    score[np.arange(S), o["state"]] = 40.0
    peaked = _numpy(sections.sections(ens, x, y, Z1_LINE, draws=R, seed=5, score=torch.as_tensor(score).to(_dev())))
    same = np.all(peaked["draw_state"] == peaked["state"][None, :], axis=1)
    print("peaked score: %d of %d realisations are the Viterbi path" % (int(same.sum()), R))
    assert same.sum() >= R // 2
    for r in range(R):
        total, size = _path_terms(peaked["draw_state"][r], score, g, d2, partner)
        assert peaked["draw_log_score"][r, 0] <= peaked["log_score"][0] + S * U * size
        if same[r]:
            assert abs(peaked["draw_log_score"][r, 0] - peaked["log_score"][0]) <= S * U * size
    lp = peaked["log_partition"][0]                                            # a log probability: <= 0 up to the rounding of sum ln s (every s > 1 here)
    assert np.all(peaked["draw_log_score"][:, 0] - lp <= 16.0 * U * (S + abs(lp)) + S * U * abs(lp))


def test_draws_of_real_chains():
    B, nk, thin, R = 16, 32, 2, 8
    _, _, dc = _chains(B, 17, exact=True, hitmap=True, ensemble=dict(n_keep=nk, thin=thin))
    dc.run(60, accumulate=False)
    dc.run(nk * thin)
    z1 = float(dc.n_depth_bins * dc.depth_bin_width)
    ens = ensembles.from_chains(dc)
    kk = ens.k.clone()
    kk[3] = 0                                                                  # a sounding without models cuts its sequence
    ens = ens._replace(k=kk)
    x, y, ptr = 20.0 * np.arange(B), np.zeros(B), np.array([0, 7, B])
    out = sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, draws=R, seed=11)
    o = _numpy(out)
    k, edges, sigma = (a.cpu().numpy() for a in (ens.k, ens.edges, ens.sigma))
    at = np.nonzero(np.arange(B) != 3)[0]
    assert o["draw_state"].shape == (R, B) and o["draw_slot"].shape == (R, B) and o["draw_log_score"].shape == (R, 2)
    assert np.all(o["draw_state"][:, 3] == -1) and np.all(o["draw_slot"][:, 3] == -1)
    assert np.all(o["draw_state"][:, at] >= 0) and np.all(o["draw_state"][:, at] < 16)
    assert np.array_equal(o["draw_slot"][:, at], o["rows"][at[None, :], o["draw_state"][:, at]]) and np.all(k[at[None, :], o["draw_slot"][:, at]] > 0)
    # the models: bit copies, and the raster of the gathered models
    depth_edges = np.linspace(0.0, z1, 25)
    models = sections.draw_models(ens, out["draw_slot"], depth_edges=depth_edges, log10=False)
    m = _numpy(models)
    assert m["k"].shape == (R, B) and m["edges"].shape == (R, B, edges.shape[2]) and m["raster"].shape == (R, B, 24)
    assert np.all(m["k"][:, 3] == 0) and np.isnan(m["edges"][:, 3]).all() and np.isnan(m["sigma"][:, 3]).all() and np.isnan(m["raster"][:, 3]).all()
    assert np.array_equal(m["k"][:, at], k[at[None, :], o["draw_slot"][:, at]])
    assert np.array_equal(m["edges"][:, at].view(np.int64), edges[at[None, :], o["draw_slot"][:, at]].view(np.int64))
    assert np.array_equal(m["sigma"][:, at].view(np.int64), sigma[at[None, :], o["draw_slot"][:, at]].view(np.int64))
    every = ensembles.realisations(ens, depth_edges, log10=False).cpu().numpy()      # [B, n_keep, n_depth]
    assert np.array_equal(m["raster"][:, at].view(np.int64), every[at[None, :], o["draw_slot"][:, at]].view(np.int64))
    assert "raster" not in sections.draw_models(ens, out["draw_slot"])
    # one run per launch: the same draws
    small = _numpy(sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, draws=R, seed=11, budget_bytes=9 * 16 * 16 * 8))
    assert all(np.array_equal(small[name], o[name], equal_nan=True) for name in o)
    quick = sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, draws=R, seed=11, marginals=False)      # draws without the marginals
    assert "weight" not in quick and torch.equal(quick["draw_state"], out["draw_state"]) and torch.equal(quick["draw_log_score"], out["draw_log_score"])
    fewer = sections.sections(ens, x, y, z1, ptr=ptr, max_models=16, draws=3, seed=11)
    assert torch.equal(fewer["draw_state"], out["draw_state"][:3])
    # the rule on the device's distances, run by run; the key of a sounding is its index in the survey
    partner = sections.partners(ptr, o["n_used"])
    d2 = sections.cross_distance(ens, out["rows"], partner, 0.0, z1).cpu().numpy()
    g = sections.steps(x, y, ptr=ptr)
    sums = np.zeros((R, 2))
    for (a, b), owner in (((0, 3), 0), ((4, 7), 0), ((7, B), 1)):
        ref = sections.draw_reference([0, b - a], None, g[a:b], d2[a:b], o["n_used"][a:b], R, seed=11, row_key=np.arange(a, b))
        _check_draws(o["draw_state"][:, a:b], ref, np.array([0, b - a]), o["n_used"][a:b], "real chains, run %d .. %d" % (a, b))
        for r in range(R):
            total, size = _path_terms(o["draw_state"][r, a:b], None, g[a:b], d2[a:b], np.where(partner[a:b] >= 0, partner[a:b] - a, -1))
            sums[r, owner] += total
    assert np.all(np.abs(o["draw_log_score"] - sums) <= B * U * np.abs(sums))      # every term has one sign: sum |terms| = |sum|
    assert np.all(o["draw_log_score"] <= o["log_score"][None, :] + B * U * np.abs(sums))
    # the area of the section more conductive than the ensemble's median, within a window
    threshold = float(np.nanmedian(sigma[k > 0]))
    area = sections.exceedance_area(models["k"], models["edges"], models["sigma"], x, y, ptr, threshold, 5.0, 0.5 * z1)
    want = sections.exceedance_area_reference(m["k"], m["edges"], m["sigma"], x, y, ptr, threshold, 5.0, 0.5 * z1)
    n_terms = np.diff(ptr) * edges.shape[2]
    print("exceedance area: %.4g .. %.4g m^2" % (want.min(), want.max()))
    assert area.shape == (R, 2) and area.device.type == "cuda" and want.max() > 0 and np.ptp(want) > 0
    assert np.all(np.abs(area.cpu().numpy() - want) <= n_terms[None, :] * U * want)          # the terms are areas: sum |terms| = the sum
    below = sections.exceedance_area(models["k"], models["edges"], models["sigma"], x, y, ptr, threshold, 5.0, 0.5 * z1, above=False).cpu().numpy()
    width = sections.section_widths(x, y, ptr)
    whole = np.array([width[0:7][np.arange(0, 7) != 3].sum(), width[7:].sum()]) * (0.5 * z1 - 5.0)
    assert np.allclose(area.cpu().numpy() + below, whole[None, :], rtol=1e-12, atol=0)       # above and below fill the window where there are models


def test_from_survey_and_the_command_line_with_draws(tmp_path):
    from geobipy_amd import survey
    res = survey.infer(os.path.join(GOLDEN, "resolve_options_small"), exact_jacobian=True, ensemble=16)
    z1 = 120.0
    direct = sections.from_survey(res, z1, z0=2.0, measure="log", tau=0.2, draws=4, seed=3)
    path = str(tmp_path / "survey.npz")
    res.save(path)
    loaded = sections.from_survey(path, z1, z0=2.0, measure="log", tau=0.2, draws=4, seed=3)
    written = sections.main([path, "--depth", "120", "--from", "2", "--measure", "log", "--tau", "0.2", "--draws", "4", "--seed", "3"])
    f, d, l = sections.load(written), _numpy(direct), _numpy(loaded)
    S, L = res["line"].size, sections.line_ptr(res["line"]).size - 1
    assert set(f) == set(d) == set(l) and {"draw_state", "draw_slot", "draw_log_score", "state", "weight"} <= set(f)
    for name in d:
        assert np.array_equal(f[name], d[name], equal_nan=True) and np.array_equal(l[name], d[name], equal_nan=True), name
    assert d["draw_state"].shape == (4, S) and d["draw_slot"].shape == (4, S) and d["draw_log_score"].shape == (4, L)
    assert np.array_equal(d["draw_state"] >= 0, np.tile(d["state"] >= 0, (4, 1)))
    other = _numpy(sections.from_survey(res, z1, z0=2.0, measure="log", tau=0.2, draws=4, seed=4))
    assert not np.array_equal(other["draw_state"], d["draw_state"]) and np.array_equal(other["state"], d["state"])
    no = sections.load(sections.main([path, "--depth", "120", "--no-marginals", "--draws", "4"]))
    assert "weight" not in no and no["draw_state"].shape == (4, S) and no["draw_log_score"].shape == (4, L)
    assert "draw_state" not in sections.load(sections.main([path, "--depth", "120"]))


def test_the_c_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    T, L, n, R = 3, 2, 5, 4
    ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device=dev)
    nu = torch.full((T,), n, dtype=torch.int32, device=dev)
    score, g, d2 = (torch.zeros(shape, dtype=torch.float64, device=dev) for shape in ((T, n), (T,), (T, n, n)))
    key = torch.arange(T, dtype=torch.int64, device=dev)
    fl, sc = torch.full((T, n), 7.0, dtype=torch.float64, device=dev), torch.full((T,), 7.0, dtype=torch.float64, device=dev)
    ds = torch.full((R, T), 7, dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    draw = lambda L_=L, ptr_=ptr, T_=T, n_=n, nu_=nu, score_=score, g_=g, d2_=d2, key_=key, seed=1, R_=R, fl_=fl, sc_=sc, ds_=ds: \
        lib.gbp_section_draw(L_, p(ptr_), T_, n_, p(nu_), p(score_), p(g_), p(d2_), p(key_), seed, R_, p(fl_), p(sc_), p(ds_), st)      # noqa: E731
    for kw in (dict(L_=-1), dict(n_=0), dict(n_=1025), dict(R_=0), dict(R_=65537), dict(R_=-1), dict(T_=1), dict(T_=2 ** 62), dict(T_=2 ** 50, n_=1, R_=65536),
               dict(ptr_=None), dict(nu_=None), dict(score_=None), dict(g_=None), dict(d2_=None), dict(fl_=None), dict(sc_=None), dict(ds_=None)):
        assert draw(**kw) != 0 and b"gbp_section_draw" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    assert torch.all(fl == 7.0) and torch.all(sc == 7.0) and torch.all(ds == 7)      # nothing was written
    assert draw(L_=0, ptr_=None, nu_=None) == 0                            # no sequence: OK without a launch
    torch.cuda.synchronize()
    assert torch.all(ds == 7)
    assert draw(key_=None) == 0                                            # a NULL row_key is the row index
    torch.cuda.synchronize()
    by_index = ds.clone()
    assert draw() == 0
    torch.cuda.synchronize()
    assert torch.equal(ds, by_index) and bool((ds >= 0).all()) and bool((ds < n).all()) and bool((sc != 7.0).all())
