"""The per-chain algebra of the sampler's Newton and accept stages (geobipy_amd/csrc/gbp_rjmcmc.h: newton_body / newton8_core,
accept_body / accept8_body) stated once more in numpy long double (63-bit mantissa on x86), with Cholesky and the substitutions
written out as loops -- np.linalg refuses the type.  Everything that enters is fp64 (the buffers of gbp_rj_chains, the option
constants, the normals and the uniform of tests/rj_emul.py) and is widened exactly; nothing here calls rjmcmc.py or rj_emul.py,
so the three statements of the rule (device, fp64 twin, this one) only share their inputs.  Test infrastructure only.

Also the seeded input recipes both tiers of the comparison draw from (tests/test_rjmcmc_algebra.py on the host,
tests/test_rjmcmc_algebra_gpu.py on the device)."""
import math

import numpy as np

import rj_emul

LD = np.longdouble
EPS = 2.0 ** -52
NONE, INSERT, DELETE, PERTURB = 0, 1, 2, 3
LOG_2PI = np.log(LD(2) * np.arctan(LD(1)) * LD(4))
MEAN_LIMIT = 11356.0            # |reverse mean| at or beyond it: the ratio is NaN (the reference's long-double exp over / underflows)


def ld(a):
    return np.asarray(a, dtype=LD)


def prior_operator(o, edges_r, k):
    """Wm'Wm [k, k]: value_precision I + gradient_precision Wz'Wz with Wz of RectilinearMesh1D.gradient_operator -- rows
    (-1, 1) / (centre-to-centre distance x (k - 1)); the half-space below the last interface counts with the first layer's width
    when k == 2 and with (last finite width + depth of the last interface) otherwise; k == 1: Wz = [[1]]."""
    op = np.zeros((k, k), dtype=LD)
    op[np.arange(k), np.arange(k)] = LD(o["value_precision"])
    if not o["solve_gradient"]:
        return op
    gp = LD(o["gradient_precision"])
    if k == 1:
        op[0, 0] += gp
        return op
    e = ld(edges_r)[: k - 1]
    x = np.empty(k, dtype=LD)
    x[: k - 1] = np.diff(np.concatenate([ld([0.0]), e]))
    x[k - 1] = x[0] if k == 2 else x[k - 2] + e[k - 2]
    t2 = gp / (LD(0.5) * (x[:-1] + x[1:]) * LD(k - 1)) ** 2
    for j in range(k - 1):
        op[j, j] += t2[j]
        op[j + 1, j + 1] += t2[j]
        op[j, j + 1] -= t2[j]
        op[j + 1, j] -= t2[j]
    return op


def variances(data, rel, add, rel_group=None, add_group=None, add_scale=None):
    """(rel_g d)^2 + (add_g' add_scale)^2 per channel."""
    data, rel, add = ld(data), np.atleast_1d(ld(rel)), np.atleast_1d(ld(add))
    r = rel[np.asarray(rel_group)] if rel_group is not None else rel[0]
    a = add[np.asarray(add_group)] if add_group is not None else add[0]
    if add_scale is not None:
        a = a * ld(add_scale)
    return (r * data) ** 2 + a ** 2 + np.zeros(data.shape, dtype=LD)


def cholesky(H):
    k = H.shape[0]
    C = np.zeros((k, k), dtype=LD)
    for j in range(k):
        C[j, j] = np.sqrt(H[j, j] - C[j, :j] @ C[j, :j])
        if j + 1 < k:
            C[j + 1:, j] = (H[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    return C


def solve_lower(C, b):                       # C y = b
    y = np.zeros(b.size, dtype=LD)
    for j in range(b.size):
        y[j] = (b[j] - C[j, :j] @ y[:j]) / C[j, j]
    return y


def solve_upper(C, b):                       # C' y = b
    y = np.zeros(b.size, dtype=LD)
    for j in range(b.size - 1, -1, -1):
        y[j] = (b[j] - C[j + 1:, j] @ y[j + 1:]) / C[j, j]
    return y


def newton_parts(o, edges_r, sigma_r, J, pred, data, rel, add, z, log_mean, rel_group=None, add_group=None, add_scale=None):
    """Everything of the Newton stage for one chain: H = J'PJ + Wm'Wm over the active channels (data > 0), g, C with H = C C',
    x = H^-1 g, w = C^-T z, log_prop = ln sigma_r - alpha x + w; and the magnitudes the tests' rounding bounds are made of."""
    k = len(sigma_r)
    a = np.asarray(data) > 0.0
    Ja = ld(J)[a][:, :k]
    P = 1 / variances(data, rel, add, rel_group, add_group, add_scale)[a]
    op = prior_operator(o, edges_r, k)
    H = op + Ja.T @ (P[:, None] * Ja)
    ls = np.log(ld(sigma_r))
    g = op @ (ls - LD(log_mean)) + Ja.T @ (P * (ld(pred)[a] - ld(data)[a]))
    C = cholesky(H)
    x = solve_upper(C, solve_lower(C, g))
    w = solve_upper(C, ld(z)[:k])
    alpha = LD(o["alpha"])
    return dict(log_prop=ls - alpha * x + w, C=C, H=H, g=g, x=x, w=w,
                H_abs=np.abs(op) + np.abs(Ja).T @ (P[:, None] * np.abs(Ja)),         # sum of |terms| of every entry of H
                M=np.abs(ls) + np.abs(alpha * x) + np.abs(w))


def newton(o, edges_r, sigma_r, J, pred, data, rel, add, z, log_mean, rel_group=None, add_group=None, add_scale=None):
    """(log_prop, C, H) of the stochastic-Newton proposal of one chain.  o: value_precision, gradient_precision, solve_gradient,
    alpha; z: the k normals."""
    p = newton_parts(o, edges_r, sigma_r, J, pred, data, rel, add, z, log_mean, rel_group, add_group, add_scale)
    return p["log_prop"], p["C"], p["H"]


def levels_log_prior(x, lo, hi):
    """Sum of the log-uniform densities of the levels, -inf outside; with the sum of the terms' magnitudes."""
    x, lo, hi = np.atleast_1d(ld(x)), np.atleast_1d(ld(lo)), np.atleast_1d(ld(hi))
    lx, llo, lhi = np.log(x), np.log(lo), np.log(hi)
    if not np.all((lx >= llo) & (lx <= lhi)):
        return LD(-np.inf), LD(0)
    t = -np.log(lhi - llo)
    return t.sum(), np.abs(t).sum()


def accept_parts(o, action, edges_r, sigma_r, thk_r, log_prop, C, J_p, pred_p, data, rel_p, add_p, prior, like, log_mean,
                 like_p=None, misfit_p=None, sigma_p=None, rel_group=None, add_group=None, add_scale=None):
    """The accept stage for one chain.  o: the keys of newton plus max_layers, solve_value, limits (or None), rel_min / rel_max /
    add_min / add_max.  log_prop, C: what the Newton stage left (fp64 buffers); like_p / misfit_p: planted for the moves that keep
    the dimension (their likelihood comes from the fused forward kernel), computed here from pred_p for a jump; sigma_p: the
    buffer parameter_limits is tested on (default exp(log_prop))."""
    k = len(sigma_r)
    lpv = ld(log_prop)[:k]
    vprec, gprec = LD(o["value_precision"]), LD(o["gradient_precision"])
    prior_p = -np.log(LD(o["max_layers"]) - 1)
    mags = {"prior": np.abs(prior_p)}
    if o.get("solve_value"):
        d2 = ((lpv - LD(log_mean)) ** 2).sum()
        t = [-LD(0.5) * k * LOG_2PI, LD(0.5) * k * np.log(vprec), -LD(0.5) * vprec * d2]
        prior_p += sum(t)
        mags["prior"] += sum(abs(v) for v in t)
    if o["solve_gradient"]:
        gr = np.diff(lpv) / np.log(ld(thk_r)[: k - 1])
        n = max(1, k - 1)
        t = [-LD(0.5) * n * LOG_2PI, LD(0.5) * n * np.log(gprec), -LD(0.5) * gprec * (gr * gr).sum()]
        prior_p += sum(t)
        mags["prior"] += sum(abs(v) for v in t)
    if o.get("limits") is not None:
        sp = np.exp(lpv) if sigma_p is None else ld(sigma_p)[:k]
        if not np.all((sp >= LD(o["limits"][0])) & (sp <= LD(o["limits"][1]))):
            prior_p = LD(-np.inf)
    for x, lo, hi in ((rel_p, o["rel_min"], o["rel_max"]), (add_p, o["add_min"], o["add_max"])):
        t, m = levels_log_prior(x, lo, hi)
        prior_p += t
        mags["prior"] += m
    dq, mean_r = LD(0), None
    mags["dq"] = LD(0)
    jump = action in (INSERT, DELETE)
    if jump:
        a = np.asarray(data) > 0.0
        var = variances(data, rel_p, add_p, rel_group, add_group, add_scale)[a]
        r = ld(pred_p)[a] - ld(data)[a]
        s2 = (r * r / var).sum()
        logdet = np.log(var).sum()
        na = LD(int(a.sum()))
        misfit_p = s2
        like_p = -(LD(0.5) * na) * LOG_2PI - LD(0.5) * logdet - LD(0.5) * s2
        mags["like"] = LD(0.5) * na * LOG_2PI + LD(0.5) * np.abs(np.log(var)).sum() + LD(0.5) * s2
        Cl = np.tril(ld(C)[:k, :k])
        op = prior_operator(o, edges_r, k)
        grad = op @ (lpv - LD(log_mean)) + ld(J_p)[a][:, :k].T @ (r / var)
        mean_r = lpv + LD(o["alpha"]) * solve_upper(Cl, solve_lower(Cl, grad))
        lrem = np.log(ld(sigma_r))
        q1, q2 = ((Cl.T @ (lrem - mean_r)) ** 2).sum(), ((Cl.T @ (lpv - lrem)) ** 2).sum()
        dq = -LD(0.5) * q1 + LD(0.5) * q2
        mags["dq"] = LD(0.5) * (q1 + q2)
        if not np.all(np.abs(mean_r) < MEAN_LIMIT):
            dq = LD(np.nan)
    else:
        like_p, misfit_p = LD(like_p), LD(misfit_p)
        mags["like"] = np.abs(like_p)
    log_ratio = (prior_p - LD(prior)) + (like_p - LD(like)) + dq
    mags["ratio"] = mags["prior"] + abs(LD(prior)) + mags["like"] + abs(LD(like)) + mags["dq"]
    return dict(log_ratio=log_ratio, prior_p=prior_p, like_p=like_p, misfit_p=misfit_p, dq=dq, mean_r=mean_r, mags=mags)


def accept(*args, **kw):
    """(log_ratio, prior_p, like_p, misfit_p, dq, mean_r): see accept_parts."""
    p = accept_parts(*args, **kw)
    return p["log_ratio"], p["prior_p"], p["like_p"], p["misfit_p"], p["dq"], p["mean_r"]


def normals(seed, chain, it, k):
    """The k normals of stream 1 the Newton stage draws (counter j -> normals 2j, 2j + 1), fp64."""
    return np.array([v for j in range((k + 1) // 2) for v in rj_emul.normal_pair(seed, chain, it, 1, j)])[:k]


def log_uniform(seed, chain, it):
    """ln u of the Metropolis test (stream 2, counter 0), fp64 uniform widened before the logarithm."""
    r = rj_emul.philox(seed, chain, it, 2, 0)
    with np.errstate(divide="ignore"):
        return np.log(LD(rj_emul.u53(r[0], r[1])))


def cond2(H):
    return float(np.linalg.cond(np.asarray(H, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------------------------
# input recipes
# ------------------------------------------------------------------------------------------------------------------
BOUNDS = dict(rel_min=0.001, rel_max=0.5, add_min=3.0, add_max=20.0)       # priors of the error levels (Resolve's options file)
RECIPES = ("usual", "collinear", "thin", "stiff")


def draw_chain(rng, recipe, k, K, N, Gr=1, Ga=1, jscale=None, inactive=False, kind=NONE, maps=None):
    """One chain's planted inputs for both stages (fp64).  k: layers of the remapped model; kind: the move.  Jacobians and
    predictions come in three draws -- carried (J, pred), remapped (J_r, pred_r), proposal (J_p, pred_p) -- of full width K, so a
    stage that reads the wrong buffer or a column at or beyond k is seen."""
    assert recipe in RECIPES
    widths = rng.uniform(1.05, 1.2, k - 1) if recipe == "thin" else np.r_[rng.uniform(1.8, 14.3, min(1, k - 1)), rng.uniform(1.5, 14.0, max(0, k - 2))]
    edges_r = np.cumsum(widths)                                                       # (thk_r: their differences, as the proposal stage forms them)
    sigma_r = 10.0 ** rng.uniform(-3, 0, k)
    stiff = recipe == "stiff"
    data = 10.0 ** rng.uniform(2, 4, N) if stiff else 10.0 ** rng.uniform(1.3, 3.5, N)
    data[rng.uniform(size=N) < 0.2] = -1.0                                            # inactive channels
    if inactive:
        data[:] = -1.0
    if stiff:
        levels = lambda: (np.full(Gr, 0.0012) * rng.uniform(1.0, 1.05, Gr), np.full(Ga, 3.05) * rng.uniform(1.0, 1.05, Ga))
    else:
        levels = lambda: (rng.uniform(0.01, 0.4, Gr), rng.uniform(3.05, 19.5, Ga))

    def jac():
        if recipe in ("collinear", "stiff"):
            sc = (400.0 if stiff else (20.0 if k > N else 40.0)) if jscale is None else jscale
            return sc * np.outer(rng.normal(size=N), 10.0 ** rng.uniform(-3, 0, K)) + 1e-4 * rng.normal(size=(N, K))
        # (more layers than channels: the scale halved, which keeps cond(H) and with it the twin's own error in log_ratio inside the
        #  guard under which decisions are compared -- tests/test_rjmcmc_algebra.py)
        return ((20.0 if k > N else 40.0) if jscale is None else jscale) * rng.normal(size=(N, K))

    rel, add = levels()
    # (the proposal's levels and Jacobian near the remapped model's, as the sampler has them -- other values in every entry, though)
    rel_p = np.clip(rel * np.exp(0.02 * rng.normal(size=Gr)), 1.001 * BOUNDS["rel_min"], 0.999 * BOUNDS["rel_max"])
    add_p = np.clip(add * np.exp(0.02 * rng.normal(size=Ga)), 1.001 * BOUNDS["add_min"], 0.999 * BOUNDS["add_max"])
    rg_, ag_, sc_ = maps if maps is not None else (np.zeros(N, dtype=int), np.zeros(N, dtype=int), 1.0)
    # predictions a standard deviation or so from the data, as a chain in equilibrium has them (chi^2 about N)
    pred = lambda r_, a_: np.abs(data) + np.sqrt((r_[rg_] * data) ** 2 + (a_[ag_] * sc_) ** 2) * rng.normal(size=N)
    J_r = jac()
    J_p = J_r * (1.0 + 0.05 * rng.normal(size=(N, K)))
    return dict(k=k, action=int(kind), edges_r=edges_r, sigma_r=sigma_r, thk_r=np.diff(np.r_[0.0, edges_r]), data=data, rel=rel, add=add, rel_p=rel_p,
                add_p=add_p, J=jac(), J_r=J_r, J_p=J_p, pred=pred(rel, add), pred_r=pred(rel, add), pred_p=pred(rel_p, add_p),
                log_mean=math.log(10.0 ** rng.uniform(-2.0, -0.5)), recipe=recipe)


def group_maps(rng, N, Gr, Ga):
    """Channel -> level maps and the additive scale of a block with several error groups (every group used)."""
    if Gr == 1 and Ga == 1:
        return None, None, None
    rg, ag = np.arange(N) % Gr, (np.arange(N) // 2) % Ga
    return rng.permutation(rg).astype(np.int32), rng.permutation(ag).astype(np.int32), 10.0 ** rng.uniform(-0.5, 0.5, N)


def newton_inputs(ch):
    """(J, pred) the Newton stage reads: the remapped model's when the move changed the structure, the carried ones otherwise."""
    return (ch["J_r"], ch["pred_r"]) if ch["action"] != NONE else (ch["J"], ch["pred"])


# ------------------------------------------------------------------------------------------------------------------
# cases: the blocks both tiers run (shapes chosen for the launch-shape borders of the two stages)
# ------------------------------------------------------------------------------------------------------------------
SEED, ITERATION, CHAIN0 = 20260, 17, 4100          # the key of the streams: (SEED, CHAIN0 + chain index, ITERATION)
FACTOR, GRADIENT_STD = 10.0, 1.5


def case_options(K, **kw):
    """Options-file keys of a case (rjmcmc_gpu.DeviceChains(**options)) -- Resolve's, with the case's layer limit."""
    o = dict(solve_gradient=True, maximum_number_of_layers=K, minimum_depth=0.1, maximum_depth=200.0, minimum_thickness=1.0,
             initial_relative_error=0.05, minimum_relative_error=BOUNDS["rel_min"], maximum_relative_error=BOUNDS["rel_max"],
             initial_additive_error=5.0, minimum_additive_error=BOUNDS["add_min"], maximum_additive_error=BOUNDS["add_max"],
             relative_error_proposal_variance=1e-6, additive_error_proposal_variance=1e-6, probability_of_birth=1.0 / 6.0,
             probability_of_death=1.0 / 6.0, probability_of_perturb=1.0 / 6.0, probability_of_no_change=0.5, factor=FACTOR,
             gradient_standard_deviation=GRADIENT_STD, covariance_scaling=1.0)
    o.update(kw)
    return o


def rule_options(options, Gr, Ga):
    """The constants of the rule from the options-file keys, formed as rjmcmc_gpu.DeviceChains forms them (fp64 inputs)."""
    return dict(max_layers=int(options["maximum_number_of_layers"]), alpha=float(options["covariance_scaling"]),
                value_precision=1.0 / math.log(1.0 + options["factor"]) ** 2,
                gradient_precision=1.0 / options["gradient_standard_deviation"] ** 2,
                solve_gradient=bool(options["solve_gradient"]), solve_value=bool(options.get("solve_parameter", False)),
                limits=options.get("parameter_limits"),
                rel_min=np.full(Gr, options["minimum_relative_error"]), rel_max=np.full(Gr, options["maximum_relative_error"]),
                add_min=np.full(Ga, options["minimum_additive_error"]), add_max=np.full(Ga, options["maximum_additive_error"]))


def _moves(K, ks):
    """A move for every chain, cycling through the four where the layer count allows it (k: layers AFTER the remap)."""
    out = []
    for b, k in enumerate(ks):
        want = (NONE, INSERT, DELETE, PERTURB)[b % 4]
        if (want == INSERT and k < 2) or (want == DELETE and k > K - 1) or (want == PERTURB and k < 2):
            want = NONE if k < 2 else INSERT
        out.append(want)
    return out


#   name: (K, N, Gr, Ga, recipes, layer counts after the remap [, moves] [, options] [, jscale])
def _case_table():
    r3 = ("usual", "collinear", "thin")
    t = {}
    for K, N in ((2, 1), (2, 7), (7, 1), (7, 7)):                    # max_layers below the group width, N below one trip
        t["small_K%d_N%d" % (K, N)] = dict(K=K, N=N, ks=[1 + b % K for b in range(13)], recipes=r3)
    # groups of 8 chains = packed workgroups: [all k <= 2] [all k <= 4, a 3 and a 4 among them] [a k in 5..8] [k <= 8 mixed with 9 and 30]
    # [deep only] [1..8] [8s and 9s] [30s] and a last one of three chains (idle groups) that holds a deep chain of the SECOND scanning
    # workgroup (rows 64..66)
    ks = ([1, 2, 2, 1, 2, 1, 2, 2] + [2, 3, 1, 4, 2, 4, 3, 1] + [2, 1, 6, 3, 2, 8, 1, 4] + [3, 9, 8, 30, 1, 9, 5, 30]
          + [9, 12, 30, 17, 10, 29, 9, 24] + [1, 2, 3, 4, 5, 6, 7, 8] + [8, 9, 8, 9, 8, 9, 8, 9] + [30, 30, 2, 30, 2, 30, 4, 30] + [5, 30, 2])
    t["waves_K30_N12"] = dict(K=30, N=12, ks=ks, recipes=r3, edges=True)
    for N in (33, 45):                                               # second 32-channel trip, pick4, variance_at
        t["groups_K16_N%d" % N] = dict(K=16, N=N, Gr=2, Ga=2, ks=[1, 8, 9, 16, 2, 5, 12, 3, 16, 7, 10, 4, 6], recipes=r3)
    for N in (64, 65):                                               # the 64-stride loops at their border
        t["stride_K9_N%d" % N] = dict(K=9, N=N, Gr=4, Ga=4, ks=[1, 9, 8, 2, 9, 5, 3, 9, 7, 4, 6, 8, 9], recipes=r3)
    for N in (130, 256):                                             # lanes 32..63, 64-lane sums, largest LDS blocks
        t["deep_K64_N%d" % N] = dict(K=64, N=N, ks=[1, 8, 9, 33, 63, 64, 64, 33, 9, 8, 1, 63, 2, 34, 64, 5, 32, 63, 9, 8, 64], recipes=r3,
                                      edges=(N == 130))
    # the 8-layer border: 8 -> 9 births and 9 -> 8 deaths (the wave-per-chain body's) next to 8 -> 8, 7 -> 8, 8 -> 7 (packed) and 9 -> 9
    ks = [9, 8, 8, 9, 8, 7, 9, 8, 8, 9, 9, 8, 8, 8, 9, 8, 7, 9, 9, 8, 8, 9, 8, 8, 9, 8, 9]
    mv = [INSERT, DELETE, PERTURB, PERTURB, INSERT, DELETE, INSERT, DELETE, NONE, NONE, INSERT, DELETE, PERTURB, INSERT, DELETE, DELETE,
          DELETE, PERTURB, INSERT, PERTURB, DELETE, DELETE, INSERT, NONE, INSERT, DELETE, PERTURB]
    t["border_K30_N12"] = dict(K=30, N=12, ks=ks, moves=mv, recipes=r3)
    t["priors_K12_N12"] = dict(K=12, N=12, ks=[1, 2, 12, 8, 9, 3, 11, 5, 4, 10, 6, 7, 8, 9, 2, 12, 3, 11, 5], recipes=r3, limit_chains=(4, 7),
                               options=dict(solve_parameter=True, solve_gradient=False, parameter_limits=[1e-12, 1e9]))
    t["stiff_K8_N12"] = dict(K=8, N=12, ks=[8, 8, 7, 8, 5, 8, 6, 8, 8, 4, 8, 7, 8], recipes=("stiff",), jscale=400.0)
    t["stiff_K30_N12"] = dict(K=30, N=12, ks=[30, 9, 30, 16, 8, 30, 24, 12, 30, 8, 30, 20, 30], recipes=("stiff",), jscale=400.0)
    return t


CASES = _case_table()
_built = {}


def build_case(name):
    """The planted block of a case, with the long-double rule's results for every chain: the Newton stage's from the planted
    inputs, the accept stage's from the Newton results rounded to fp64 (so each stage is tested on its own).  The carried prior
    is set so that log_ratio - ln u straddles zero at margins between 1e-7 and 1.  Cached: built once per process."""
    if name in _built:
        return _built[name]
    spec = CASES[name]
    K, N, Gr, Ga = spec["K"], spec["N"], spec.get("Gr", 1), spec.get("Ga", 1)
    rng = np.random.default_rng([SEED, sorted(CASES).index(name)])
    options = case_options(K, **spec.get("options", {}))
    o = rule_options(options, Gr, Ga)
    rel_group, add_group, add_scale = group_maps(rng, N, Gr, Ga)
    maps = dict(rel_group=rel_group, add_group=add_group, add_scale=add_scale)
    ks = spec["ks"]
    moves = spec.get("moves") or _moves(K, ks)
    B = len(ks)
    assert B % 8 != 0
    # the planted edge paths: an all-inactive jump (every case); with edges=True also a jump whose reverse mean leaves +-11356
    jumps = [b for b in range(B) if moves[b] in (INSERT, DELETE)]
    inactive = jumps[len(jumps) // 2]
    huge = [b for b in jumps if b != inactive and ks[b] <= 8][:1] + [b for b in jumps if b != inactive and ks[b] > 8][:1] if spec.get("edges") else []
    chains = []
    for b, k in enumerate(ks):
        ch = draw_chain(rng, spec["recipes"][b % len(spec["recipes"])], k, K, N, Gr, Ga, spec.get("jscale"), b == inactive, moves[b],
                        None if rel_group is None else (rel_group, add_group, add_scale))
        ch["b"], ch["chain_id"] = b, CHAIN0 + b
        ch["edge"] = "inactive" if b == inactive else ("mean" if b in huge else ("limits" if b in spec.get("limit_chains", ()) else None))
        if ch["edge"] == "mean":
            ch["J_p"] = ch["J_p"] * 1e9
        if ch["edge"] == "limits":
            ch["sigma_r"] = ch["sigma_r"] * 1e12
        # the carried model the move started from
        e, s, a = ch["edges_r"], ch["sigma_r"], ch["action"]
        if a == INSERT:
            i = int(rng.integers(1, k))
            ch["edges"], ch["sigma"] = np.delete(e, i - 1), np.delete(s, i)
        elif a == DELETE:
            i = int(rng.integers(1, k + 1))
            top, bot = (e[i - 2] if i > 1 else 0.0), (e[i - 1] if i < k else (e[-1] if k > 1 else 0.0) + 6.0)
            ch["edges"], ch["sigma"] = np.insert(e, i - 1, 0.5 * (top + bot)), np.insert(s, i, s[i - 1] * 1.5)
        else:
            ch["edges"], ch["sigma"] = e.copy(), s.copy()
        z = normals(SEED, ch["chain_id"], ITERATION, k)
        Jn, pn = newton_inputs(ch)
        ch["z"] = z
        ch["newton"] = nw = newton_parts(o, e, s, Jn, pn, ch["data"], ch["rel"], ch["add"], z, ch["log_mean"], **maps)
        # what the accept stage finds in the Newton stage's buffers
        ch["log_prop"], ch["chol"] = np.asarray(nw["log_prop"], dtype=np.float64), np.asarray(nw["C"], dtype=np.float64)
        ch["sigma_p"] = np.asarray(np.exp(ld(ch["log_prop"])), dtype=np.float64)
        std = np.sqrt(np.asarray(variances(ch["data"], ch["rel"], ch["add"], **maps), dtype=np.float64))
        act = ch["data"] > 0.0
        r = (ch["pred"][act] - ch["data"][act]) / std[act]
        ch["misfit"] = float(np.sum(r * r))
        ch["like"] = float(-(0.5 * act.sum()) * math.log(2.0 * math.pi) - np.sum(np.log(std[act])) - 0.5 * ch["misfit"])
        # (the planted likelihood of a proposal that keeps its dimension: what the fused forward kernel would have left)
        std_p = np.sqrt(np.asarray(variances(ch["data"], ch["rel_p"], ch["add_p"], **maps), dtype=np.float64))
        r = (ch["pred_p"][act] - ch["data"][act]) / std_p[act]
        ch["misfit_p"] = float(np.sum(r * r))
        ch["like_p"] = float(-(0.5 * act.sum()) * math.log(2.0 * math.pi) - np.sum(np.log(std_p[act])) - 0.5 * ch["misfit_p"])
        ch["ln_u"] = log_uniform(SEED, ch["chain_id"], ITERATION)
        args = (o, a, e, s, ch["thk_r"], ch["log_prop"], ch["chol"], ch["J_p"], ch["pred_p"], ch["data"], ch["rel_p"], ch["add_p"])
        kw = dict(log_mean=ch["log_mean"], like_p=ch["like_p"], misfit_p=ch["misfit_p"], sigma_p=ch["sigma_p"], **maps)
        free = accept_parts(*args, prior=0.0, like=ch["like"], **kw)           # log_ratio + the carried prior
        sign, margin = (1.0 if (b % 2 or b == inactive) else -1.0), 10.0 ** rng.uniform(-7.0, 0.0)      # (the all-inactive jump is accepted)
        lr0 = free["log_ratio"]
        ch["prior"] = float(lr0 - ch["ln_u"] - LD(sign * margin)) if np.isfinite(lr0) else -50.0 - b
        ch["accept"] = acc = accept_parts(*args, prior=ch["prior"], like=ch["like"], **kw)
        with np.errstate(invalid="ignore"):
            ch["accepted"] = bool(ch["ln_u"] < acc["log_ratio"])
            ch["margin"] = float(abs(ch["ln_u"] - acc["log_ratio"]))
        chains.append(ch)
    case = dict(name=name, K=K, N=N, Gr=Gr, Ga=Ga, B=B, options=options, o=o, chains=chains, **maps)
    _built[name] = case
    return case


def twin_priors(case, ch):
    """(sp, vp) of tests/rj_emul.py / rjmcmc.py for a chain of a case."""
    from geobipy_amd import rjmcmc
    op = case["options"]
    sp = rjmcmc.StructurePrior(case["K"], op["minimum_depth"], op["maximum_depth"], op["minimum_thickness"], [1, 1, 1, 3])
    vp = rjmcmc.ValuePrior(math.exp(ch["log_mean"]), op["factor"], op["gradient_standard_deviation"], op["solve_gradient"],
                           bool(op.get("solve_parameter", False)), op.get("parameter_limits"))
    return sp, vp


def twin_newton(case, ch):
    """rj_emul.newton on a chain of a case: (log_prop, C) in fp64."""
    _, vp = twin_priors(case, ch)
    Jn, pn = newton_inputs(ch)
    grouped = case["rel_group"] is not None
    rel, add = (ch["rel"], ch["add"]) if grouped else (ch["rel"][0], ch["add"][0])
    return rj_emul.newton(dict(alpha=case["o"]["alpha"]), SEED, ch["chain_id"], ITERATION, vp, ch["edges_r"], ch["sigma_r"], Jn, pn, ch["data"],
                          rel, add, 1.0 if not grouped else case["add_scale"], (case["rel_group"], case["add_group"]) if grouped else None)


def twin_accept(case, ch):
    """rj_emul.accept on a chain of a case, fed with the same planted buffers as the rule: (log_ratio, accepted, prior_p)."""
    from geobipy_amd import rjmcmc
    sp, vp = twin_priors(case, ch)
    grouped = case["rel_group"] is not None
    groups = (case["rel_group"], case["add_group"]) if grouped else None
    scale = case["add_scale"] if grouped else 1.0
    rel_p, add_p = (ch["rel_p"], ch["add_p"]) if grouped else (ch["rel_p"][0], ch["add_p"][0])
    like_p = ch["like_p"]
    if ch["action"] in (INSERT, DELETE):
        like_p = rjmcmc.gauss_loglike(ch["pred_p"], ch["data"], rj_emul.channel_std(ch["data"], rel_p, add_p, scale, groups))[1]
    o = case["o"]
    eo = dict(alpha=o["alpha"], rel_min=o["rel_min"], rel_max=o["rel_max"], add_min=o["add_min"], add_max=o["add_max"])
    with np.errstate(all="ignore"):
        return rj_emul.accept(eo, SEED, ch["chain_id"], ITERATION, sp, vp, ch["action"], ch["edges_r"], ch["sigma_r"], ch["log_prop"], ch["chol"],
                              ch["J_p"], ch["pred_p"], ch["data"], rel_p, add_p, like_p, ch["prior"], ch["like"], scale, groups)
