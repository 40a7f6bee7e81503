"""The sampler's Newton and accept stages, host tier: the long-double statement of the rule (tests/rj_longdouble.py) against
the fp64 twin (tests/rj_emul.py) on every planted block the device tier runs (tests/test_rjmcmc_algebra_gpu.py), its own
consistency, closed forms, and the guards of the input recipes -- conditions on the REFERENCE alone, so the device tier's bars
(max(16 e, rounding bound) with e the twin's distance from the rule) cannot hide behind a wide e.  No GPU.

Measured here (docs/notes_sampler_algebra.md has the table): e(log_prop) <= 2e-11 for the usual / collinear / thin recipes up to
k = 64, N = 256, 2e-10 .. 3e-10 for the stiff one (cond(H) up to 2e6); e(log_ratio) <= 4e-12 outside the stiff recipe, up to
2e-7 inside it -- which is why decisions are compared outside it only."""
import numpy as np
import pytest

import rj_longdouble as R
from rj_longdouble import LD, EPS, INSERT, DELETE

CASE_NAMES = sorted(R.CASES)
DECISION_GUARD, USUAL_GUARD, STIFF_GUARD = 1e-10, 1e-9, 1e-6      # caps on 16 e


def twin_distances(case):
    """Per chain: e(log_prop), e(C) / max|C|, e(log_ratio) of the fp64 twin against the rule, and cond2(H)."""
    out = []
    for ch in case["chains"]:
        nw, ac = ch["newton"], ch["accept"]
        lp, C = R.twin_newton(case, ch)
        lr, acc, prior_p = R.twin_accept(case, ch)
        with np.errstate(invalid="ignore"):
            e_ratio = float(abs(LD(lr) - ac["log_ratio"])) if np.isfinite(ac["log_ratio"]) else 0.0
        same_kind = (np.isnan(lr) and np.isnan(ac["log_ratio"])) or (np.isneginf(lr) and np.isneginf(ac["log_ratio"])) or np.isfinite(lr)
        out.append(dict(e_lp=float(np.max(np.abs(ld_(lp) - nw["log_prop"]))), e_C=float(np.max(np.abs(ld_(C) - nw["C"])) / np.max(np.abs(nw["C"]))),
                        e_ratio=e_ratio, cond=R.cond2(nw["H"]), twin_accepted=acc, same_kind=bool(same_kind),
                        e_prior=float(abs(LD(prior_p) - ac["prior_p"])) if np.isfinite(ac["prior_p"]) else 0.0))
    return out


def ld_(a):
    return np.asarray(a, dtype=LD)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_twin_and_rule_are_the_same_function(name):
    """e <= 64 k cond2(H) 2^-52 max(1, |log_prop|_inf) for the proposal, likewise for C relative to max|C|: the twin's distance from
    the rule is rounding of a backward-stable fp64 solve, nothing else.  And the recipes' guards."""
    case = R.build_case(name)
    dist = twin_distances(case)
    stiff = name.startswith("stiff")
    for ch, d in zip(case["chains"], dist):
        k = ch["k"]
        bar = 64.0 * k * d["cond"] * EPS
        lp_inf = max(1.0, float(np.max(np.abs(ch["newton"]["log_prop"]))))
        print("%s b=%d k=%d %s move %d cond %.1e  e(log_prop) %.2e/%.2e  e(C) %.2e/%.2e  e(log_ratio) %.2e" % (
            name, ch["b"], k, ch["recipe"], ch["action"], d["cond"], d["e_lp"], bar * lp_inf, d["e_C"], bar, d["e_ratio"]))
        assert d["e_lp"] <= bar * lp_inf and d["e_C"] <= bar, (name, ch["b"])
        assert d["same_kind"], (name, ch["b"])                       # NaN where the rule has NaN, -inf where it has -inf
        assert 16.0 * d["e_lp"] <= (STIFF_GUARD if stiff else USUAL_GUARD), (name, ch["b"], d["e_lp"])
        if not stiff:                                                # decisions are compared here (test_rjmcmc_algebra_gpu.py)
            assert 16.0 * d["e_ratio"] <= DECISION_GUARD, (name, ch["b"], d["e_ratio"])
            if ch["margin"] >= 1e-9:
                assert d["twin_accepted"] == ch["accepted"], (name, ch["b"])
    conds = [d["cond"] for d in dist]
    print("%s: max e(log_prop) %.2e  max e(log_ratio) %.2e  cond %.1e .. %.1e" % (
        name, max(d["e_lp"] for d in dist), max(d["e_ratio"] for d in dist), min(conds), max(conds)))
    if stiff:
        assert 1e5 <= max(conds) <= 1e7, conds                       # the recipe reaches the conditioning it is there for, and stops there


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rule_is_consistent_in_long_double(name):
    """C C' = H entry by entry to k 2^-60 of sqrt(H_ii H_jj), and H x = g to k 2^-60 of |H| |x| + |g| (infinity norms): the loops
    written out in tests/rj_longdouble.py factor and solve what they say."""
    case = R.build_case(name)
    for ch in case["chains"]:
        nw, k = ch["newton"], ch["k"]
        H, C, x, g = nw["H"], nw["C"], nw["x"], nw["g"]
        d = np.sqrt(np.diag(H))
        r1 = float(np.max(np.abs(C @ C.T - H) / np.outer(d, d)))
        r2 = float(np.max(np.abs(H @ x - g)) / (np.max(np.abs(H).sum(axis=1)) * np.max(np.abs(x)) + np.max(np.abs(g)) + LD(1e-300)))
        tol = k * 2.0 ** -60
        assert np.array_equal(np.triu(C, 1), np.zeros_like(C)) and np.all(np.diag(C) > 0)
        assert r1 <= tol and r2 <= tol, (name, ch["b"], k, r1, r2, tol)
        w = nw["w"]
        assert float(np.max(np.abs(C.T @ w - ld_(ch["z"])[:k]))) <= tol * float(np.max(np.abs(C)) * np.max(np.abs(w)) + 1.0)


def test_closed_forms():
    rng = np.random.default_rng(5)
    o = R.rule_options(R.case_options(12), 1, 1)
    # k = 1: C = sqrt(value_precision + gradient_precision + sum P J^2), log_prop = ln sigma - alpha g / H + z / C
    for N, alpha in ((1, 1.0), (12, 0.7)):
        ch = R.draw_chain(rng, "usual", 1, 12, N)
        oo = dict(o, alpha=alpha)
        z = np.array([0.37])
        lp, C, H = R.newton(oo, ch["edges_r"], ch["sigma_r"], ch["J"], ch["pred"], ch["data"], ch["rel"], ch["add"], z, ch["log_mean"])
        a = ch["data"] > 0
        P = 1 / ((LD(ch["rel"][0]) * ld_(ch["data"])) ** 2 + LD(ch["add"][0]) ** 2)[a]
        J0 = ld_(ch["J"])[a, 0]
        h = LD(o["value_precision"]) + LD(o["gradient_precision"]) + (P * J0 * J0).sum()
        g = (LD(o["value_precision"]) + LD(o["gradient_precision"])) * (np.log(LD(ch["sigma_r"][0])) - LD(ch["log_mean"])) \
            + (J0 * P * (ld_(ch["pred"])[a] - ld_(ch["data"])[a])).sum()
        want = np.log(LD(ch["sigma_r"][0])) - LD(alpha) * g / h + LD(z[0]) / np.sqrt(h)
        assert abs(C[0, 0] - np.sqrt(h)) <= 4 * 2.0 ** -63 * np.sqrt(h) and abs(lp[0] - want) <= 2.0 ** -58 * max(1.0, abs(want))
    # every channel inactive: H is the prior operator (tridiagonal), and a jump's likelihood and misfit are exact zeros
    for k, recipe in ((2, "usual"), (3, "thin"), (9, "usual"), (30, "collinear")):
        ch = R.draw_chain(rng, recipe, k, 30, 12, inactive=True, kind=INSERT)
        z = R.normals(3, 9, 1, k)
        nw = R.newton_parts(o, ch["edges_r"], ch["sigma_r"], ch["J_r"], ch["pred_r"], ch["data"], ch["rel"], ch["add"], z, ch["log_mean"])
        op = R.prior_operator(o, ch["edges_r"], k)
        assert np.array_equal(nw["H"], op) and np.array_equal(op, op.T)
        i, j = np.indices(op.shape)
        assert not op[np.abs(i - j) > 1].any() and np.all(op[np.abs(i - j) == 1] < 0)
        # rows of Wz'Wz sum to zero: what is left of a row's sum is value_precision
        assert float(np.max(np.abs(op.sum(axis=1) - LD(o["value_precision"])))) <= 8 * 2.0 ** -63 * float(np.max(np.abs(op)))
        # against rjmcmc.py's operator, to fp64 rounding
        from geobipy_amd import rjmcmc
        vp = rjmcmc.ValuePrior(np.exp(ch["log_mean"]), R.FACTOR, R.GRADIENT_STD, True)
        ref = rjmcmc.model_prior_derivative(vp, ch["edges_r"], ch["sigma_r"], 2)
        assert np.allclose(np.asarray(op, dtype=np.float64), ref, rtol=16 * EPS * k, atol=0.0)
        acc = R.accept_parts(o, INSERT, ch["edges_r"], ch["sigma_r"], ch["thk_r"], np.asarray(nw["log_prop"], dtype=np.float64),
                             np.asarray(nw["C"], dtype=np.float64), ch["J_p"], ch["pred_p"], ch["data"], ch["rel_p"], ch["add_p"], prior=-3.0, like=0.0,
                             log_mean=ch["log_mean"])
        assert acc["like_p"] == 0 and acc["misfit_p"] == 0 and np.isfinite(acc["log_ratio"])
    # alpha = 0: the mean of the proposal is ln sigma
    ch = R.draw_chain(rng, "collinear", 7, 12, 12)
    z = R.normals(3, 10, 1, 7)
    nw = R.newton_parts(dict(o, alpha=0.0), ch["edges_r"], ch["sigma_r"], ch["J"], ch["pred"], ch["data"], ch["rel"], ch["add"], z, ch["log_mean"])
    assert np.array_equal(nw["log_prop"], np.log(ld_(ch["sigma_r"])) + nw["w"])
    lp0, _, _ = R.newton(dict(o, alpha=0.0), ch["edges_r"], ch["sigma_r"], ch["J"], ch["pred"], ch["data"], ch["rel"], ch["add"], np.zeros(7), ch["log_mean"])
    assert np.array_equal(lp0, np.log(ld_(ch["sigma_r"])))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_planted_blocks_reach_what_they_are_for(name):
    """Accepts and rejects each take at least 20 % of a block, both happen among the jumps, every decision's margin is at least
    1e-7 wide (so none is left out of the device comparison at 1e-9), about a fifth of the channels is inactive, one chain has
    none active, the error levels are inside their priors, and the planted edge paths are where the rule says."""
    case = R.build_case(name)
    chains, B = case["chains"], case["B"]
    acc = np.array([ch["accepted"] for ch in chains])
    jump = np.array([ch["action"] in (INSERT, DELETE) for ch in chains])
    assert B % 8 != 0 and B % 64 != 0
    assert acc.sum() >= 0.2 * B and (~acc).sum() >= 0.2 * B and (acc & jump).any() and (~acc & jump).any()
    plain = [ch for ch in chains if ch["edge"] not in ("mean", "limits")]
    assert all(1e-7 * (1 - 1e-3) <= ch["margin"] <= 1.0 + 1e-3 for ch in plain), [ch["margin"] for ch in plain]
    frac = np.mean([np.mean(ch["data"] <= 0) for ch in chains if ch["edge"] != "inactive"])
    assert case["N"] < 7 or 0.1 < frac < 0.3, frac
    assert sum(ch["edge"] == "inactive" for ch in chains) == 1
    b = R.BOUNDS
    for ch in chains:
        for key in ("rel", "rel_p"):
            assert np.all((ch[key] > b["rel_min"]) & (ch[key] < b["rel_max"]))
        for key in ("add", "add_p"):
            assert np.all((ch[key] > b["add_min"]) & (ch[key] < b["add_max"]))
        a = ch["accept"]
        if ch["edge"] == "inactive":
            assert ch["action"] in (INSERT, DELETE) and not (ch["data"] > 0).any() and a["like_p"] == 0 and a["misfit_p"] == 0
        elif ch["edge"] == "mean":                                   # far beyond the limit, not at it
            assert np.isnan(a["log_ratio"]) and float(np.max(np.abs(a["mean_r"]))) > 100 * R.MEAN_LIMIT and not ch["accepted"]
        elif ch["edge"] == "limits":
            assert np.isneginf(a["log_ratio"]) and not ch["accepted"]
            assert float(np.min(ch["sigma_p"][: ch["k"]])) > 10 * case["o"]["limits"][1] or float(np.max(ch["sigma_p"][: ch["k"]])) > 10 * case["o"]["limits"][1]
        else:
            assert np.isfinite(a["log_ratio"])
            if a["mean_r"] is not None:
                assert float(np.max(np.abs(a["mean_r"]))) < 0.01 * R.MEAN_LIMIT
            if case["o"]["limits"] is not None:
                sp = ch["sigma_p"][: ch["k"]]
                assert np.all((sp > 10 * case["o"]["limits"][0]) & (sp < 0.1 * case["o"]["limits"][1]))
    if "edges" in R.CASES[name] and R.CASES[name]["edges"]:
        ks = sorted(ch["k"] for ch in chains if ch["edge"] == "mean")
        assert len(ks) == 2 and ks[0] <= 8 < ks[1]                    # one for the packed body, one for the wave-per-chain body
