"""The sampler's Newton and accept stages (gbp_rj_newton / gbp_rj_accept, geobipy_amd/csrc/gbp_rjmcmc.h) on planted blocks against
the rule in long double (tests/rj_longdouble.py), at the launch-shape borders of both stages: max_layers below the packed group
width, waves of the packed body that take its 2-, 4- and 8-column instantiations, identity rows and idle groups, the packed and
the wave-per-chain body in one launch and the 8-layer border between them, N across the 8-, 32- and 64-channel trips up to 256,
2 and 4 error groups with maps and add_scale, K = 64, the value prior / parameter_limits branches, and an ill-conditioned recipe.

Every bar is max(16 e, a derived rounding bound): e is the distance of the fp64 twin (tests/rj_emul.py) from the rule over the
case's chains of the same body -- held under the caps of tests/test_rjmcmc_algebra.py on the host -- and the rounding bound is
stated where it is used.  Every number is printed as used/bar.  docs/notes_sampler_algebra.md has the measured table."""
import types

import numpy as np
import pytest
import torch

import rj_longdouble as R
from rj_longdouble import LD, EPS, NONE, INSERT, DELETE, PERTURB
from geobipy_amd import rjmcmc_gpu as rg

pytestmark = pytest.mark.gpu
CASE_NAMES = sorted(R.CASES)
FILL = -7.0


class _NoSystem:
    """Neither stage entry evaluates physics: a system without a handle."""
    def handle(self):
        return types.SimpleNamespace(ptr=None, bins=None)


class PlantedChains(rg.DeviceChains):
    """The product's own filling of gbp_rj_options / gbp_rj_chains for any (B, K, N, groups); the state is planted afterwards."""
    def _initialize(self):
        pass


def _block(case):
    B, N = case["B"], case["N"]
    return PlantedChains(_NoSystem(), np.full(B, 30.0), np.ones((B, N)), seed=R.SEED, rel_group=case["rel_group"], add_group=case["add_group"],
                         add_scale=case["add_scale"], chain_id=np.arange(B) + R.CHAIN0, **case["options"])


def _rows(case, order, stage):
    """The planted arrays [B, ...] with the case's chain order[r] in row r.  stage "newton": the stage's outputs hold FILL;
    "accept": they hold the rule's Newton results rounded to fp64."""
    K, N, Gr, Ga, B = case["K"], case["N"], case["Gr"], case["Ga"], case["B"]
    f = lambda *s, v=0.0: np.full(s, v, dtype=np.float64)
    a = dict(chain_id=np.zeros(B, dtype=np.int64), data=f(B, N), log_mean_prior=f(B), k=np.zeros(B, dtype=np.int32), edges=f(B, K, v=np.inf),
             sigma=f(B, K, v=1.0), rel=f(B, Gr), add=f(B, Ga), pred=f(B, N), J=f(B, N, K), prior=f(B), like=f(B), misfit=f(B),
             action=np.zeros(B, dtype=np.int32), k_r=np.zeros(B, dtype=np.int32), edges_r=f(B, K, v=np.inf), sigma_r=f(B, K, v=1.0), thk_r=f(B, K),
             rel_p=f(B, Gr), add_p=f(B, Ga), pred_r=f(B, N), J_r=f(B, N, K), chol=f(B, K, K, v=FILL), log_prop=f(B, K, v=FILL),
             sigma_p=f(B, K, v=FILL), pred_p=f(B, N), misfit_p=f(B, v=FILL), like_p=f(B, v=FILL), J_p=f(B, N, K), log_ratio=f(B, v=FILL),
             n_accepted=np.zeros(B, dtype=np.int64), best_posterior=f(B))
    for r, b in enumerate(order):
        ch = case["chains"][b]
        k, kc = ch["k"], len(ch["sigma"])
        a["chain_id"][r], a["data"][r], a["log_mean_prior"][r] = ch["chain_id"], ch["data"], ch["log_mean"]
        a["k"][r], a["edges"][r, : kc - 1], a["sigma"][r, :kc] = kc, ch["edges"], ch["sigma"]
        a["k_r"][r], a["action"][r] = k, ch["action"]
        a["edges_r"][r, : k - 1], a["sigma_r"][r, :k], a["thk_r"][r, : k - 1] = ch["edges_r"], ch["sigma_r"], ch["thk_r"]
        for n in ("rel", "add", "rel_p", "add_p", "pred", "pred_r", "pred_p", "J", "J_r", "J_p", "prior", "like", "misfit"):
            a[n][r] = ch[n]
        a["best_posterior"][r] = ch["prior"] + ch["like"]
        if stage == "accept":
            a["chol"][r][np.tril_indices(k)] = ch["chol"][np.tril_indices(k)]
            a["log_prop"][r], a["sigma_p"][r] = 0.0, 1.0
            a["log_prop"][r, :k], a["sigma_p"][r, :k] = ch["log_prop"], ch["sigma_p"]
            if ch["action"] not in (INSERT, DELETE):             # (a jump's likelihood is the stage's own: its slots keep FILL)
                a["like_p"][r], a["misfit_p"][r] = ch["like_p"], ch["misfit_p"]
    return a


def _plant(dc, arrays):
    for n, v in arrays.items():
        dc.t[n].copy_(torch.as_tensor(v))
    for n in ("k_hist", "edge_hist", "rel_hist", "add_hist", "step_flags"):
        dc.t[n].zero_()
    torch.cuda.synchronize()


def _run(dc, stage):
    from geobipy_amd import _lib
    lib = _lib.load()
    if stage == "newton":
        _lib.check(lib.gbp_rj_newton(dc._o, dc._c, R.ITERATION, None))
    else:
        _lib.check(lib.gbp_rj_accept(dc._o, dc._c, R.ITERATION, 0, None))
    torch.cuda.synchronize()
    return {n: dc.t[n].cpu().numpy().copy() for n in ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "action", "k_r",
                                                      "edges_r", "sigma_r", "thk_r", "rel_p", "add_p", "pred_r", "J_r", "chol", "log_prop", "sigma_p",
                                                      "pred_p", "misfit_p", "like_p", "J_p", "log_ratio", "n_accepted", "best_posterior", "k_hist",
                                                      "data", "log_mean_prior", "chain_id")}


def _same(x, y):
    return np.array_equal(x, y, equal_nan=(x.dtype.kind == "f"))


def _instantiations(case, order, stage):
    """What every packed workgroup (8 rows) and every scanning workgroup (64 rows) of the launch is expected to run."""
    ch, B = case["chains"], case["B"]
    lines = []
    for w in range((B + 7) // 8):
        rows = [ch[b] for b in order[8 * w: 8 * w + 8]]
        if stage == "newton":
            mine = [c["k"] for c in rows if c["k"] <= 8]
        else:
            mine = [c["k"] for c in rows if max(c["k"], len(c["sigma"])) <= 8 and c["action"] in (INSERT, DELETE)]
        km = 8 if any(k > 4 for k in mine) else (4 if any(k > 2 for k in mine) else (2 if (mine or stage == "newton") else 0))
        what = "newton8_core<%d>" % km if stage == "newton" else ("accept8_reverse<%d>" % km if km else "accept8_body, no packed jump")
        lines.append("packed wg %d: k_r %s -> %s%s" % (w, [c["k"] for c in rows], what, ", %d idle groups" % (8 - len(rows)) if len(rows) < 8 else ""))
    if case["K"] > 8:
        for w in range((B + 63) // 64):
            deep = [r for r in range(64 * w, min(B, 64 * w + 64)) if _deep(ch[order[r]], stage)]
            lines.append("scanning wg %d: rows %s -> %s" % (w, deep, "newton_body" if stage == "newton" else "accept_body"))
    return lines


def _deep(ch, stage):
    return ch["k"] > 8 if stage == "newton" else max(ch["k"], len(ch["sigma"])) > 8


_twin = {}


def _twin_distances(case):
    """e(log_prop) and e(log_ratio) of the fp64 twin against the rule: per chain, and the largest per body of each stage."""
    if case["name"] not in _twin:
        e_lp, e_lr = [], []
        for ch in case["chains"]:
            lp, _ = R.twin_newton(case, ch)
            e_lp.append(float(np.max(np.abs(np.asarray(lp, dtype=LD) - ch["newton"]["log_prop"]))))
            lr = R.twin_accept(case, ch)[0]
            e_lr.append(float(abs(LD(lr) - ch["accept"]["log_ratio"])) if np.isfinite(ch["accept"]["log_ratio"]) else 0.0)
        body = lambda stage, deep, e: max([v for ch, v in zip(case["chains"], e) if _deep(ch, stage) == deep], default=0.0)
        _twin[case["name"]] = dict(newton={d: body("newton", d, e_lp) for d in (False, True)}, accept={d: body("accept", d, e_lr) for d in (False, True)})
    return _twin[case["name"]]


def _orders(B):
    """Row orders of the three runs: as drawn (twice), and every chain at another row, in other company."""
    return list(range(B)), list(range(B)), [(5 * r + 3) % B for r in range(B)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_newton_stage_against_the_rule(name):
    case = R.build_case(name)
    K, N, B = case["K"], case["N"], case["B"]
    e_body = _twin_distances(case)["newton"]
    dc = _block(case)
    outs = []
    for order in _orders(B):
        arrays = _rows(case, order, "newton")
        _plant(dc, arrays)
        outs.append((order, arrays, _run(dc, "newton")))
    order, arrays, out = outs[0]
    print("\n".join(_instantiations(case, order, "newton")))
    worst = dict(factor=0.0, log_prop=0.0, sigma_p=0.0, distance=0.0)
    for r, b in enumerate(order):
        ch = case["chains"][b]
        k, nw = ch["k"], ch["newton"]
        chol, lp, sp = out["chol"][r], out["log_prop"][r], out["sigma_p"][r]
        low = np.tril(np.ones((K, K), dtype=bool))
        low[k:, :] = False
        assert np.all(chol[~low] == FILL), (name, b, "entries above the diagonal and rows >= k keep the fill")
        # factor: Higham's componentwise bound for Cholesky, |C C' - H| <= (k + 1) u |C||C'| with (|C||C'|)_ij <= sqrt(H_ii H_jj) (1 + O(u)),
        # plus the rounding of forming H from N + 3 terms per entry: (N + 4) u sum_n |terms|_ij.  Nothing measured in it.
        Cd = np.asarray(np.tril(chol[:k, :k]), dtype=LD)
        H, d = nw["H"], np.sqrt(np.diag(nw["H"]))
        bar = ((k + 2) + (N + 4)) * EPS * (np.outer(d, d) + nw["H_abs"])
        used = float(np.max(np.abs(Cd @ Cd.T - H) / bar))
        # log_prop: 16 x the twin's own distance from the rule over the chains of this body, or the rounding of the stage's last
        # sums -- N + 4 k + 16 roundings of magnitude M = |ln sigma| + alpha |x| + |w| -- whichever is larger
        bar_lp = np.maximum(16.0 * e_body[k > 8], (N + 4 * k + 16) * EPS * np.asarray(nw["M"], dtype=np.float64))
        dist = np.abs(np.asarray(lp[:k], dtype=LD) - nw["log_prop"])
        used_lp = float(np.max(dist / bar_lp))
        # sigma_p: exp of the stage's own log_prop to 2 ulp
        want = np.exp(np.asarray(lp[:k], dtype=LD))
        used_sp = float(np.max(np.abs(np.asarray(sp[:k], dtype=LD) - want) / (2.0 * np.spacing(sp[:k]))))
        print("%s b=%d k=%d %s: factor %.3f/1  log_prop %.3f/1 (bar %.2e, e %.2e)  sigma_p %.3f/1" % (
            name, b, k, "deep" if k > 8 else "packed", used, used_lp, float(np.max(bar_lp)), e_body[k > 8], used_sp))
        assert used <= 1.0 and used_lp <= 1.0 and used_sp <= 1.0, (name, b, k, used, used_lp, used_sp)
        assert not lp[k:].any() and np.all(sp[k:] == 1.0), (name, b, "zeros / ones behind k")
        worst = dict(factor=max(worst["factor"], used), log_prop=max(worst["log_prop"], used_lp), sigma_p=max(worst["sigma_p"], used_sp),
                     distance=max(worst["distance"], float(np.max(dist))))
    print("%s newton: worst used/bar  factor %.3f  log_prop %.3f  sigma_p %.3f   e packed %.2e deep %.2e   largest |log_prop - rule| %.2e" % (
        name, worst["factor"], worst["log_prop"], worst["sigma_p"], e_body[False], e_body[True], worst["distance"]))
    # the stage writes nothing but its three outputs
    for n, v in arrays.items():
        if n not in ("chol", "log_prop", "sigma_p"):
            assert _same(out[n], v), (name, n)
    # the same block twice: the same bits; the same chains at other rows, in other waves: the same bits
    for n in ("chol", "log_prop", "sigma_p"):
        assert _same(outs[1][2][n], out[n]), (name, n, "run twice")
        moved = outs[2][2][n]
        for r2, b in enumerate(outs[2][0]):
            assert _same(moved[r2], out[n][b]), (name, n, b, "moved to row %d" % r2)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_accept_stage_against_the_rule(name):
    case = R.build_case(name)
    K, N, B = case["K"], case["N"], case["B"]
    stiff = name.startswith("stiff")
    e_body = _twin_distances(case)["accept"]
    dc = _block(case)
    outs = []
    for order in _orders(B):
        arrays = _rows(case, order, "accept")
        _plant(dc, arrays)
        outs.append((order, arrays, _run(dc, "accept")))
    order, arrays, out = outs[0]
    print("\n".join(_instantiations(case, order, "accept")))
    n_acc = n_rej = left_out = 0
    jump_acc = jump_rej = False
    worst = dict(log_ratio=0.0, prior=0.0, like=0.0, misfit=0.0, distance=0.0)
    for r, b in enumerate(order):
        ch = case["chains"][b]
        k, ac, mags, action = ch["k"], ch["accept"], ch["accept"]["mags"], ch["action"]
        jump = action in (INSERT, DELETE)
        deep = _deep(ch, "accept")
        lr = out["log_ratio"][r]
        accepted = int(out["n_accepted"][r]) == 1
        assert int(out["n_accepted"][r]) in (0, 1)
        n_acc += accepted
        n_rej += not accepted
        jump_acc |= jump and accepted
        jump_rej |= jump and not accepted
        roundings = (N + 4 * k + 32) * EPS            # the stage's sums: N channels, 4 k terms of the k-vectors, 32 for the scalar terms
        if ch["edge"] == "mean":
            assert np.isnan(lr) and not accepted, (name, b, lr)
        elif ch["edge"] == "limits":
            assert np.isneginf(lr) and not accepted, (name, b, lr)
        else:
            bar = max(16.0 * e_body[deep], roundings * float(mags["ratio"]))
            used = float(abs(LD(lr) - ac["log_ratio"])) / bar
            print("%s b=%d k=%d move %d %s: log_ratio %.3f/1 (bar %.2e, e %.2e) margin %.1e %s" % (
                name, b, k, action, "deep" if deep else "packed", used, bar, e_body[deep], ch["margin"], "accepted" if accepted else "rejected"))
            assert used <= 1.0, (name, b, k, action, lr, float(ac["log_ratio"]))
            worst["log_ratio"], worst["distance"] = max(worst["log_ratio"], used), max(worst["distance"], used * bar)
            # decisions: the rule's wherever the margin is at least 1e-9 (the host tier holds 16 e(log_ratio) <= 1e-10 there); under the
            # stiff recipe, whose twin is itself up to 2e-7 away, wherever the margin is beyond twice the bar just asserted
            if ch["margin"] >= (max(1e-9, 2.0 * bar) if stiff else 1e-9):
                assert accepted == ch["accepted"], (name, b, lr, float(ch["ln_u"]), float(ac["log_ratio"]))
            else:
                left_out += 1
        row = lambda n: out[n][r]
        if accepted:
            for got, want, mag, what in ((row("prior"), ac["prior_p"], mags["prior"], "prior"), (row("like"), ac["like_p"], mags["like"], "like"),
                                         (row("misfit"), ac["misfit_p"], ac["misfit_p"], "misfit")):
                if jump or what == "prior":
                    if float(mag) == 0.0:
                        assert got == 0.0, (name, b, what)
                        continue
                    used = float(abs(LD(got) - want)) / (roundings * float(mag))
                    assert used <= 1.0, (name, b, what, got, float(want), used)
                    worst[what] = max(worst[what], used)
                else:
                    assert got == arrays[what + "_p"][r], (name, b, what)      # planted by the forward kernel's stand-in: copied
            assert row("k") == k and _same(row("edges"), arrays["edges_r"][r]) and _same(row("sigma"), arrays["sigma_p"][r]), (name, b)
            assert _same(row("pred"), arrays["pred_p"][r]) and _same(row("rel"), arrays["rel_p"][r]) and _same(row("add"), arrays["add_p"][r])
            kc = min(K, (k + 7) & ~7)                              # the columns the Jacobian pass wrote
            Jwant = arrays["J"][r].copy()
            if action != NONE:
                Jwant[:, :kc] = (arrays["J_r"] if action == PERTURB else arrays["J_p"])[r][:, :kc]
            assert _same(row("J"), Jwant), (name, b, action)
            assert row("best_posterior") == max(arrays["best_posterior"][r], row("prior") + row("like"))
        else:
            for n in ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "best_posterior"):
                assert _same(row(n), arrays[n][r]), (name, b, n, "a rejected chain is untouched")
        if ch["edge"] == "inactive":                             # (planted as an accepted jump: its likelihood is in the state)
            assert jump and accepted and row("like") == 0.0 and row("misfit") == 0.0, (name, b)
    print("%s accept: %d accepted, %d rejected, %d left out of the decisions;  worst used/bar  log_ratio %.3f  prior %.3f  like %.3f  misfit %.3f;"
          "  e packed %.2e deep %.2e   largest |log_ratio - rule| %.2e" % (name, n_acc, n_rej, left_out, worst["log_ratio"], worst["prior"], worst["like"],
                                                                          worst["misfit"], e_body[False], e_body[True], worst["distance"]))
    assert n_acc >= 0.2 * B and n_rej >= 0.2 * B and jump_acc and jump_rej
    if not stiff:
        assert left_out <= 0.01 * B
    # nothing but the chain state, the ratio and the counters is written
    for n, v in arrays.items():
        if n not in ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "log_ratio", "n_accepted", "best_posterior"):
            assert _same(out[n], v), (name, n)
    assert not out["k_hist"].any()                               # (accumulate = 0)
    # the same block twice: the same bits; the same chains at other rows, in other waves: the same bits
    for n in ("k", "edges", "sigma", "rel", "add", "pred", "J", "prior", "like", "misfit", "log_ratio", "n_accepted", "best_posterior"):
        assert _same(outs[1][2][n], out[n]), (name, n, "run twice")
        moved = outs[2][2][n]
        for r2, b in enumerate(outs[2][0]):
            assert _same(moved[r2], out[n][b]), (name, n, b, "moved to row %d" % r2)

