"""Horizon tracking along a line: the most probable path (Viterbi) and the smoothed marginals (forward-backward) of a Markov chain
over the depth cells of a window, one chain per line and horizon (csrc/gbp_horizon.h, ``gbp_horizon_track``).

The per-sounding evidence for an interface -- ``interface_probability`` of the line products, or the sampled ``first_hist`` /
``first_none`` of a threshold -- knows nothing of the neighbouring soundings, and its mode jumps from sounding to sounding.  Here the
evidence is multiplied by a Laplace prior on the change of the horizon's ELEVATION between neighbours (scale ``slope`` metres per metre
of distance), so the path is coherent under terrain, and an extra state **absent** ("no such horizon under this sounding") can be
entered and left at the price ``switch``.

The rule (``track_reference`` states it in numpy, fp64; the device is held to it: ``==`` for the path and its score, the reference's
own rounding for the marginals).  A launch holds L sequences concatenated with ``ptr`` [L + 1]; all share the S states (cells of
uniform width ``dz``, ascending depth) and whether the absent state (index S) exists.  Per step n -> n + 1 inside a sequence
g[n] = 1 / (slope max(dx_n, min_distance)) and d[n] = surface[n + 1] - surface[n] (``steps``); cell c -> cell c' costs
T_n[k] = g[n] |d[n] - k dz| with k = c' - c, cell <-> absent costs ``switch``, absent -> absent 0.

  Viterbi: V_0 = score[0]; V_{n+1}[c'] = score[n + 1, c'] + max(max_c (V_n[c] - T_n[c' - c]), V_n[absent] - switch), and for the absent
  state absent_score[n + 1] + max(max_c (V_n[c] - switch), V_n[absent]).  The maximiser is the FIRST maximum in the order c = 0 .. S - 1,
  then absent (strict > replaces); the path ends at the first maximum of V_{N-1} in the same order.
  Marginals (scaled forward-backward, linear domain): w = exp(score), K_n[k] = exp(-T_n[k]), ks = exp(-switch); alpha_0 = w_0 / s_0,
  alpha_{n+1}[c'] = w[n + 1, c'] (sum_c alpha_n[c] K_n[c' - c] + alpha_n[absent] ks), c ascending, each alpha normalised by its sum
  s_{n+1}; beta_{N-1} = 1, beta_n = K_n (w_{n+1} o beta_{n+1}) / s_{n+1}; gamma_n = alpha_n o beta_n renormalised;
  log_partition = sum_n ln s_n.

A window of depth is applied by slicing the state axis, which is exact: the costs depend on differences of cell indices only.  There
is no host fallback for ``track`` itself.

Across lines (csrc/gbp_horizon_graph.h; ``gbp_horizon_graph_propagate``, ``gbp_horizon_graph_path``,
``gbp_horizon_graph_refine``).  Lines tracked alone give stripes: where a line's evidence is bimodal along its whole length the pick
sits on the wrong branch for the entire line, and nothing inside that line can tell.  ``spatial`` puts the same states and the same
pair term on the survey graph of ``sections.neighbours`` -- the steps along every line plus, across lines, every sounding's nearest
sounding of every other line within ``max_distance`` -- with g[e] = 1 / (slope max(dist_e, min_distance)) and d[e] = surface[ev[e]] -
surface[eu[e]] of the edge (``graph_steps``).  ``propagate_reference`` states the sum-product rule (beliefs) and
``graph_path_reference`` the max-sum rule, its decode by conditioning level by level and its coordinate ascent (the most probable
horizon surface) in numpy; ``propagate``, ``graph_path`` and ``refine`` run them on the device: the max-sum side has numpy's bits, the
sum side the reference's own rounding.  On a line graph they are the chain's marginals and its Viterbi path; on a graph with loops
they are an approximation (a belief is not a marginal), and the path is never less probable than any candidate it was given -- the
lines tracked alone among them.

Joint draws (csrc/gbp_horizon_draw.h; ``gbp_horizon_draw``, ``gbp_horizon_graph_draw``).  A pick has no spread and a
marginal cannot say which depth under one sounding goes with which under the next.  ``draw_reference`` states forward filtering and
backward sampling of the chain above in numpy, ``draw`` runs it on the device, ``track(draws=R)`` and ``from_products(draws=R)`` return R
joint realisations per horizon, and ``draw_summary`` / ``connected`` turn them into posteriors of a length, a cross-section, a gap, "no
gap from a to b".  Across lines ``graph_draw_reference`` states Gibbs sampling blocked by flight line on the survey graph -- the same
filter and walk per line, its weights multiplied by the pair factors at the neighbouring lines' current states --, ``graph_draw`` runs
it, and ``spatial(draws=R)`` / ``spatial_from_products(draws=R)`` return the realisations with ``draw_share`` and
``draw_change_share``.  Where several horizons share a launch or a survey the row key of a draw is sounding index + horizon index * N.

Horizon pairs (csrc/gbp_horizon_unit.h; ``gbp_horizon_unit_track``).  Two picks tracked one by one can cross, can be
the same interface twice, and have no joint posterior, so a unit has no thickness.  ``unit_reference`` states one chain over the
ordered pairs (top, base) of cells of one window, base - top >= ``min_cells`` -- the pair term is separable, so a step is two passes
of S^3 operations --, ``unit`` and ``unit_from_products`` run it on the device and return the two picks, the thickness and its
posterior, and ``unit_intervals`` hands the unit to ``line_products``.

Left out on purpose: more than two horizons tracked jointly, pairs on the survey graph and joint draws of pairs, learning ``slope``
(``log_partition`` of ``track`` is returned for whoever wants to scan it), non-uniform depth cells, gridding the picks into a surface,
and a place in ``survey.infer``.
"""
import argparse
import os

import numpy as np
import torch

from . import _args, _lib
from ._args import first_max, load_npz as load, save_npz as save  # noqa: F401  (this module's ``save`` and ``load``)

MAX_STATES = 2048
OUTPUT_SUFFIX = ".horizons.npz"


def percentile_name(p):
    return "depth_percentile_%g" % float(p)


def check_ptr(ptr, total):
    """``ptr`` as int64 numpy [L + 1]: starts at 0, ends at ``total``, every sequence holds at least one sounding."""
    return _args.check_ptr(ptr, total, "horizons")


def steps(x, y, surface, slope=0.05, min_distance=1.0, ptr=None):
    """(g, d) float64 [N] of the steps n -> n + 1 of soundings at ``x``, ``y`` (m) on the ``surface`` elevation (m):
    g[n] = 1 / (slope max(dx_n, min_distance)) with dx_n the horizontal distance, d[n] = surface[n + 1] - surface[n].  The entry of a
    sequence's last sounding (of ``ptr``; default one sequence) is unused and holds g = 1 / (slope min_distance), d = 0."""
    x, y, s = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, surface))
    if not (x.size == y.size == s.size):
        raise ValueError("horizons.steps: x, y and surface must have one entry per sounding")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(s))):
        raise ValueError("horizons.steps: x, y and surface must be finite")
    slope, min_distance = float(slope), float(min_distance)
    if not (np.isfinite(slope) and slope > 0.0):
        raise ValueError("horizons.steps: slope must be positive")
    if not (np.isfinite(min_distance) and min_distance > 0.0):
        raise ValueError("horizons.steps: min_distance must be positive")
    N = x.size
    dx, d = np.zeros(N), np.zeros(N)
    if N > 1:
        dx[:-1] = np.hypot(np.diff(x), np.diff(y))
        d[:-1] = np.diff(s)
    if ptr is not None:
        last = check_ptr(ptr, N)[1:] - 1
        dx[last], d[last] = 0.0, 0.0
    g = 1.0 / (slope * np.maximum(dx, min_distance))
    return g, d


def evidence_scores(evidence, absent=None, floor=1e-6):
    """(score [N, S], absent_score [N] or None) of non-negative weights ``evidence`` [N, S] and optionally ``absent`` [N] (numpy or
    torch, the result is of the same kind): with Z_n = sum_c e[n, c] + absent[n], score = ln(max(e / Z_n, floor)).  A sounding with
    Z_n == 0 (an empty map, never burned in) scores 0 in every state: it says nothing, and the path passes on the prior alone."""
    floor = float(floor)
    if not 0.0 < floor < 1.0:
        raise ValueError("horizons.evidence_scores: floor must lie in (0, 1)")
    if isinstance(evidence, torch.Tensor):
        e = evidence.to(torch.float64)
        a = None if absent is None else torch.as_tensor(absent).to(e.device, torch.float64).reshape(-1)
        where, log, ones_like, clamp = torch.where, torch.log, torch.ones_like, lambda v: torch.clamp(v, min=floor)
        bad = bool((~torch.isfinite(e)).any() or (e < 0).any()) or (a is not None and bool((~torch.isfinite(a)).any() or (a < 0).any()))
    else:
        e = np.asarray(evidence, dtype=np.float64)
        a = None if absent is None else np.asarray(absent, dtype=np.float64).reshape(-1)
        where, log, ones_like, clamp = np.where, np.log, np.ones_like, lambda v: np.maximum(v, floor)
        bad = bool((~np.isfinite(e)).any() or (e < 0).any()) or (a is not None and bool((~np.isfinite(a)).any() or (a < 0).any()))
    if e.ndim != 2 or e.shape[1] < 1:
        raise ValueError("horizons.evidence_scores: evidence must be [N, S] with S >= 1")
    if a is not None and a.shape[0] != e.shape[0]:
        raise ValueError("horizons.evidence_scores: absent must hold one weight per sounding")
    if bad:
        raise ValueError("horizons.evidence_scores: the weights must be finite and non-negative")
    Z = e.sum(1) if a is None else e.sum(1) + a
    empty = Z == 0
    Zs = where(empty, ones_like(Z), Z)
    score = where(empty[:, None], 0.0 * e, log(clamp(e / Zs[:, None])))
    absent_score = None if a is None else where(empty, 0.0 * a, log(clamp(a / Zs)))
    return score, absent_score


def track_reference(ptr, score, absent_score, g, d, dz, switch, marginals=True, dtype=np.float64):
    """The rule of the module's docstring in numpy, evaluated in ``dtype`` (fp64: what the device is held to; np.longdouble: the
    yardstick of the reference's own rounding).  ``ptr`` [L + 1], ``score`` [sum N, S], ``absent_score`` [sum N] or None, ``g``, ``d``
    [sum N] (``steps``), ``dz`` > 0, ``switch`` >= 0.  Returns ``cell`` int32 [sum N] (S: absent), ``log_score`` [L], and with
    ``marginals`` ``marginal`` [sum N, S (+ 1)] (the absent state last), ``log_partition`` [L] and ``scale`` [sum N] (s_n)."""
    ft = np.dtype(dtype).type
    score = np.asarray(score, dtype=np.float64)
    if score.ndim != 2 or score.shape[1] < 1:
        raise ValueError("horizons.track_reference: score must be [N, S] with S >= 1")
    total, S = score.shape
    ptr = check_ptr(ptr, total)
    has_absent = absent_score is not None
    g, d = np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(d, dtype=np.float64).reshape(-1)
    if g.size != total or d.size != total:
        raise ValueError("horizons.track_reference: g and d must hold one entry per sounding")
    if has_absent:
        absent_score = np.asarray(absent_score, dtype=np.float64).reshape(-1)
        if absent_score.size != total:
            raise ValueError("horizons.track_reference: absent_score must hold one entry per sounding")
    if not (np.isfinite(dz) and dz > 0.0):
        raise ValueError("horizons.track_reference: dz must be positive")
    if not (np.isfinite(switch) and switch >= 0.0):
        raise ValueError("horizons.track_reference: switch must be >= 0")
    if not (np.all(np.isfinite(score)) and np.all(np.isfinite(g)) and np.all(np.isfinite(d)) and (not has_absent or np.all(np.isfinite(absent_score)))):
        raise ValueError("horizons.track_reference: the scores and steps must be finite")
    score, g, d = score.astype(ft), g.astype(ft), d.astype(ft)
    absent_score = absent_score.astype(ft) if has_absent else None
    dz, switch = ft(dz), ft(switch)
    SA, L = S + int(has_absent), ptr.size - 1
    kf = np.arange(-(S - 1), S).astype(ft)                                   # k = c' - c at index k + S - 1
    cell, log_score = np.zeros(total, dtype=np.int32), np.zeros(L, dtype=ft)
    out = dict(cell=cell, log_score=log_score)
    if marginals:
        gamma, log_partition, scale = np.zeros((total, SA), dtype=ft), np.zeros(L, dtype=ft), np.zeros(total, dtype=ft)
        out.update(marginal=gamma, log_partition=log_partition, scale=scale)
    # for a fixed c the costs of all c' are the slice [S - 1 - c, 2 S - 1 - c) of the 2 S - 1 values; for a fixed c' those of all c the
    # slice [c', c' + S) reversed: the loops below run over c (or c') ascending, as the rule's maxima and sums do
    for l in range(L):
        r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
        full = lambda n: score[r0 + n] if not has_absent else np.concatenate([score[r0 + n], absent_score[r0 + n:r0 + n + 1]])  # noqa: E731
        # ---- Viterbi
        V = full(0)
        back = np.zeros((N, SA), dtype=np.int64)
        for n in range(N - 1):
            T = g[r0 + n] * np.abs(d[r0 + n] - kf * dz)
            m, arg = np.full(S, -np.inf, dtype=ft), np.zeros(S, dtype=np.int64)
            for c in range(S):
                cand = V[c] - T[S - 1 - c:2 * S - 1 - c]
                repl = cand > m                                              # strict: the first maximum stays
                m, arg = np.where(repl, cand, m), np.where(repl, c, arg)
            nxt = np.empty(SA, dtype=ft)
            if has_absent:
                via = V[S] - switch
                repl = via > m
                arg, m = np.where(repl, S, arg), np.where(repl, via, m)
                a_arg = first_max(V[:S] - switch)
                a_m = V[a_arg] - switch
                if V[S] > a_m:
                    a_arg, a_m = S, V[S]
                nxt[S] = absent_score[r0 + n + 1] + a_m
                back[n + 1, S] = a_arg
            nxt[:S] = score[r0 + n + 1] + m
            back[n + 1, :S] = arg
            V = nxt
        cur = first_max(V)
        log_score[l] = V[cur]
        for n in range(N - 1, -1, -1):
            cell[r0 + n] = cur
            cur = back[n, cur]
        if not marginals:
            continue
        # ---- scaled forward-backward
        ks = np.exp(-switch)
        w = np.exp(np.stack([full(n) for n in range(N)]))                     # [N, SA]
        alpha = np.zeros((N, SA), dtype=ft)
        s = np.zeros(N, dtype=ft)
        s[0] = w[0].sum()
        alpha[0] = w[0] / s[0]
        Ks = []
        for n in range(N - 1):
            K = np.exp(-(g[r0 + n] * np.abs(d[r0 + n] - kf * dz)))
            Ks.append(K)
            a = alpha[n]
            u = np.zeros(SA, dtype=ft)
            for c in range(S):                                               # c ascending
                u[:S] = u[:S] + a[c] * K[S - 1 - c:2 * S - 1 - c]
            if has_absent:
                u[:S] = u[:S] + a[S] * ks
                u[S] = np.cumsum(a[:S] * ks)[-1] + a[S]
            u = w[n + 1] * u
            s[n + 1] = u.sum()
            alpha[n + 1] = u / s[n + 1]
        beta = np.ones(SA, dtype=ft)
        for n in range(N - 1, -1, -1):
            if n < N - 1:
                K = Ks[n]
                u = w[n + 1] * beta
                b = np.zeros(SA, dtype=ft)
                for c in range(S):                                           # c' ascending
                    b[:S] = b[:S] + K[c:c + S][::-1] * u[c]
                if has_absent:
                    b[:S] = b[:S] + ks * u[S]
                    b[S] = np.cumsum(ks * u[:S])[-1] + u[S]
                beta = b / s[n + 1]
            gm = alpha[n] * beta
            gamma[r0 + n] = gm / gm.sum()
        scale[r0:r0 + N] = s
        log_partition[l] = np.cumsum(np.log(s))[-1]
    return out


MAX_DRAWS = 65536


def _check_draw_chain(ptr, score, absent_score, g, d, dz, switch, n_draws, seed, row_key, what):
    """The checks ``draw_reference`` and ``draw`` share, on shapes and host values alone (``score`` numpy or torch, any device): a
    sequence of ``ptr`` may be empty.  Returns ptr (int64 numpy), g, d (float64 numpy), dz, switch, R, seed and the keys (int64 numpy;
    None when ``row_key`` is)."""
    from . import sections
    if getattr(score, "ndim", 0) != 2 or not 1 <= score.shape[1] <= MAX_STATES:
        raise ValueError("%s: score must be [N, S] with 1 <= S <= %d (choose a window with between=)" % (what, MAX_STATES))
    total = score.shape[0]
    ptr = _args.check_ptr(ptr, total, "horizons", empty=True)
    if absent_score is not None and tuple(absent_score.shape) != (total,):
        raise ValueError("%s: absent_score must hold one entry per sounding" % what)
    g, d = np.asarray(_args.host(g), dtype=np.float64).reshape(-1), np.asarray(_args.host(d), dtype=np.float64).reshape(-1)
    if g.size != total or d.size != total:
        raise ValueError("%s: g and d must hold one entry per sounding" % what)
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(d))):
        raise ValueError("%s: g and d must be finite" % what)
    dz, switch = float(dz), float(switch)
    if not (np.isfinite(dz) and dz > 0.0):
        raise ValueError("%s: dz must be positive" % what)
    if not (np.isfinite(switch) and switch >= 0.0):
        raise ValueError("%s: switch must be >= 0" % what)
    R = _args.check_int(n_draws, 1, MAX_DRAWS, "%s: n_draws" % what)
    seed = sections._check_seed(seed)
    key = None if row_key is None else sections._check_row_key(row_key, total, what)
    return ptr, g, d, dz, switch, R, seed, key


def draw_reference(ptr, score, absent_score, g, d, dz, switch, n_draws, seed=0, row_key=None, dtype=np.float64):
    """The rule of ``draw`` in numpy, evaluated in ``dtype``: joint draws of whole horizons from the chain of the module's docstring by
    forward filtering and backward sampling.  The inputs of ``track_reference`` (a sequence of ``ptr`` may be empty here), ``n_draws``
    = R in 1 .. 65536, ``seed`` (uint64) and ``row_key`` int64 [sum N] (None: the row index).

    Filter, per sequence: the forward half of ``track_reference``'s marginals, word for word -- w = exp(score), K_n[k] = exp(-(g[n] *
    |d[n] - k * dz|)), ks = exp(-switch); alpha_0 = w_0 / s_0; alpha_{n+1}[c'] = w[n + 1, c'] * (sum_c alpha_n[c] K_n[c' - c] +
    alpha_n[absent] * ks), c ascending and acc = acc + a * K; the absent row sum_c alpha_n[c] * ks + alpha_n[absent]; each row divided
    by its sum s.
    Walk: realisation rho goes n = N - 1 .. 0 over the states i = 0 .. SA - 1, cells ascending and absent last; j is the state just
    drawn under n + 1.  W[i] = alpha_n[i] at the sequence's last sounding; alpha_n[i] * K_n[j - i] for cells i and j; alpha_n[i] * ks
    for a cell i and j absent; alpha_n[S] * ks for i absent and a cell j; alpha_n[S], with no multiply, for both absent.  c =
    cumsum(W), sequential, c = c + w; thr = u * c[SA - 1]; pick = min(#{i : c[i] <= thr}, SA - 1).  A state of weight 0 is never the
    first to pass thr, so it is never drawn; with a NaN total no comparison holds and the pick is 0.
    u = ``sections.philox_uniform(seed, rho, row_key[n], sweep=0)``: a draw depends on the seed, the realisation and the sounding's key
    -- not on R, on the grouping of sequences into calls, or on a launch shape.  Where several horizons (windows, thresholds) share a
    launch or a survey, the convention is row_key = sounding index + horizon index * N, so that two horizons of one sounding never
    share a uniform.

    Returns ``draw_state`` int32 [R, sum N] (S: absent), ``filtered`` [sum N, SA] (alpha, the absent state last), ``scale`` [sum N]
    (s_n) and ``margin`` [R, L]: the smallest min_i |c[i] - thr| / c[SA - 1] over the sequence's soundings (inf for an empty sequence)
    -- how close the walk came to another outcome (a device whose exp differs in the last bit may decide a draw with a margin of a few
    ulp the other way, and the walk differs from there on)."""
    from . import sections
    what = "horizons.draw_reference"
    ft = np.dtype(dtype).type
    score = np.asarray(score, dtype=np.float64)
    has_absent = absent_score is not None
    absent_score = np.asarray(absent_score, dtype=np.float64).reshape(-1) if has_absent else None
    ptr, g, d, dz, switch, R, seed, key = _check_draw_chain(ptr, score, absent_score, g, d, dz, switch, n_draws, seed, row_key, what)
    if not (np.all(np.isfinite(score)) and (not has_absent or np.all(np.isfinite(absent_score)))):
        raise ValueError("%s: the scores must be finite" % what)
    total, S = score.shape
    key = np.arange(total, dtype=np.int64) if key is None else key
    score, g, d = score.astype(ft), g.astype(ft), d.astype(ft)
    absent_score = absent_score.astype(ft) if has_absent else None
    dz, switch = ft(dz), ft(switch)
    SA, L = S + int(has_absent), ptr.size - 1
    kf = np.arange(-(S - 1), S).astype(ft)                                   # k = c' - c at index k + S - 1
    ks = np.exp(-switch)
    rho, cells = np.arange(R, dtype=np.int64), np.arange(S, dtype=np.int64)
    draw_state, filtered, scale = np.zeros((R, total), dtype=np.int32), np.zeros((total, SA), dtype=ft), np.zeros(total, dtype=ft)
    margin = np.full((R, L), np.inf, dtype=ft)
    for l in range(L):
        r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
        if N == 0:
            continue
        full = lambda n: score[r0 + n] if not has_absent else np.concatenate([score[r0 + n], absent_score[r0 + n:r0 + n + 1]])  # noqa: E731
        w = np.exp(np.stack([full(n) for n in range(N)]))                     # [N, SA]
        alpha, s, Ks = np.zeros((N, SA), dtype=ft), np.zeros(N, dtype=ft), []
        with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
            s[0] = w[0].sum()
            alpha[0] = w[0] / s[0]
            for n in range(N - 1):
                K = np.exp(-(g[r0 + n] * np.abs(d[r0 + n] - kf * dz)))
                Ks.append(K)
                a = alpha[n]
                u = np.zeros(SA, dtype=ft)
                for c in range(S):                                           # c ascending
                    u[:S] = u[:S] + a[c] * K[S - 1 - c:2 * S - 1 - c]
                if has_absent:
                    u[:S] = u[:S] + a[S] * ks
                    u[S] = np.cumsum(a[:S] * ks)[-1] + a[S]
                u = w[n + 1] * u
                s[n + 1] = u.sum()
                alpha[n + 1] = u / s[n + 1]
            filtered[r0:r0 + N], scale[r0:r0 + N] = alpha, s
            j = None
            for n in range(N - 1, -1, -1):
                a = alpha[n]
                W = np.empty((R, SA), dtype=ft)
                if n == N - 1:
                    W[:] = a[None, :]
                else:
                    Kx = np.append(Ks[n], ks)                                # the switch in slot 2 S - 1
                    jc = j < S
                    slot = np.where(jc[:, None], j[:, None] - cells[None, :] + (S - 1), 2 * S - 1)
                    W[:, :S] = a[None, :S] * Kx[slot]
                    if has_absent:
                        W[:, S] = np.where(jc, a[S] * ks, a[S])
                c = np.cumsum(W, axis=1, dtype=ft)                           # sequential, i ascending
                thr = sections.philox_uniform(seed, rho, key[r0 + n]).astype(ft) * c[:, -1]
                j = np.minimum((c <= thr[:, None]).sum(axis=1), SA - 1)
                margin[:, l] = np.fmin(margin[:, l], np.abs(c - thr[:, None]).min(axis=1) / c[:, -1])
                draw_state[:, r0 + n] = j
    return dict(draw_state=draw_state, filtered=filtered, scale=scale, margin=margin)


def draw(ptr, score, absent_score, g, d, dz, switch, n_draws, seed=0, row_key=None):
    """Joint draws of whole horizons from the chain of ``track`` by forward filtering and backward sampling on the device
    (gbp_horizon_draw: csrc/gbp_horizon_draw.h k_horizon_filter / k_horizon_walk; ``draw_reference`` states the rule): ``score`` f64
    [sum N, S] and ``absent_score`` f64 [sum N] or None on the device, ``ptr`` [L + 1] (a sequence may be empty), ``g``, ``d`` [sum N]
    (``steps``; host or device), ``n_draws`` = R in 1 .. 65536, ``seed`` a uint64, ``row_key`` int64 [sum N] (host or device; None: the
    row index).  The uniform of realisation rho under a sounding is ``sections.philox_uniform(seed, rho, row_key)``, so soundings keep
    their draws however they are grouped into calls; where several horizons (windows, thresholds) share a launch or a survey,
    row_key = sounding index + horizon index * N keeps two horizons of one sounding from sharing a uniform.  Returns on the device
    ``draw_state`` int32 [R, sum N] (S: absent), ``filtered`` [sum N, SA] and ``scale`` [sum N].  There is no host fallback."""
    entry, what = "gbp_horizon_draw", "horizons.draw"
    _are_tensors(score, absent_score, "draw", entry)
    ptr, g, d, dz, switch, R, seed, key = _check_draw_chain(ptr, score, absent_score, g, d, dz, switch, n_draws, seed, row_key, what)
    if score.dtype != torch.float64 or (absent_score is not None and absent_score.dtype != torch.float64):
        raise TypeError("%s: score and absent_score are float64" % what)
    _args.on_device((score,) + (() if absent_score is None else (absent_score,)), "horizons", "draw", entry)
    dev = score.device
    total, S = score.shape
    L, SA = ptr.size - 1, S + (absent_score is not None)
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(draw_state=torch.empty((R, total), dtype=torch.int32, device=dev), filtered=torch.empty((total, SA), **f64),
               scale=torch.empty(total, **f64))
    if L > 0 and total > 0:
        t_key = None if key is None else torch.as_tensor(key).to(dev)
        _lib.call(entry, dev, L, torch.as_tensor(ptr).to(dev), total, int(np.diff(ptr).max()), S, dz, score.contiguous(),
                  None if absent_score is None else absent_score.contiguous(), torch.as_tensor(g).to(dev), torch.as_tensor(d).to(dev), switch, t_key,
                  seed, R, out["filtered"], out["scale"], out["draw_state"])
    return out


def draw_log_scores(draw_state, ptr, score, absent_score, g, d, dz, switch):
    """The log score of every drawn path on the scale of ``track``'s ``log_score``, f64 [R, L] on the device: per sequence the node
    terms score[n, x_n] (absent_score[n] for the absent state) summed over its soundings, minus the pair costs of its steps --
    g[n] |d[n] - (x_{n+1} - x_n) dz| between cells, ``switch`` between a cell and absent, 0 between absent and absent.  With the
    chain's ``log_partition``, ``draw_log_score - log_partition`` is the path's log probability.  Plain torch."""
    dev, (total, S) = score.device, score.shape
    x = draw_state.long()
    theta = score if absent_score is None else torch.cat([score, absent_score.reshape(-1, 1)], dim=1)
    node = theta[torch.arange(total, device=dev)[None, :], x]
    t_g, t_d = torch.as_tensor(g, dtype=torch.float64).to(dev), torch.as_tensor(d, dtype=torch.float64).to(dev)
    out = torch.zeros((x.shape[0], len(ptr) - 1), dtype=torch.float64, device=dev)
    for l in range(len(ptr) - 1):
        a, b = int(ptr[l]), int(ptr[l + 1])
        if b <= a:
            continue
        xa, xb = x[:, a:b - 1], x[:, a + 1:b]
        cost = torch.where((xa < S) & (xb < S), t_g[None, a:b - 1] * torch.abs(t_d[None, a:b - 1] - (xb - xa).to(torch.float64) * dz),
                           torch.where((xa >= S) & (xb >= S), torch.zeros((), dtype=torch.float64, device=dev),
                                       torch.full((), float(switch), dtype=torch.float64, device=dev)))
        out[:, l] = node[:, a:b].sum(dim=1) - cost.sum(dim=1)
    return out


def _draw_cells(draw_cell, n_depth, what):
    c = torch.as_tensor(draw_cell)
    if c.ndim != 2 or c.dtype.is_floating_point or c.dtype == torch.bool:
        raise ValueError("%s: draw_cell must hold integers [R, N]" % what)
    if c.numel() and (int(c.min()) < -1 or (n_depth is not None and int(c.max()) >= n_depth)):
        raise ValueError("%s: every entry of draw_cell must be -1 (absent) or a cell of the depth axis" % what)
    return c.long()


def _summary_arguments(draw_cell, depth_edges, x, y, ptr, weights, what):
    """The checked arguments of ``draw_summary`` and its reference: cells [R, N] (long), centres, widths (numpy [N]) and ptr."""
    from . import sections
    edges, _ = check_depth_edges(depth_edges)
    c = _draw_cells(draw_cell, edges.size - 1, what)
    N = c.shape[1]
    ptr = _args.check_ptr([0, N] if ptr is None else ptr, N, "horizons", empty=True)
    if weights is None:
        if np.size(x) != N or np.size(y) != N:
            raise ValueError("%s: x and y must hold one entry per sounding (%d)" % (what, N))
        width = sections.section_widths(x, y, ptr)
    else:
        width = np.asarray(_args.host(weights), dtype=np.float64).reshape(-1)
        if width.size != N or not np.all(np.isfinite(width)) or np.any(width < 0.0):
            raise ValueError("%s: weights must hold one finite non-negative weight per sounding (%d)" % (what, N))
    return c, 0.5 * (edges[1:] + edges[:-1]), width, ptr


def draw_summary_reference(draw_cell, depth_edges, x, y, ptr=None, weights=None):
    """The rule of ``draw_summary`` in numpy loops: float64 [R, L] each."""
    c, centres, width, ptr = _summary_arguments(draw_cell, depth_edges, x, y, ptr, weights, "horizons.draw_summary_reference")
    c = c.cpu().numpy()
    R, L = c.shape[0], ptr.size - 1
    out = {k: np.zeros((R, L)) for k in ("present_length", "area_above", "longest_gap")}
    for r in range(R):
        for l in range(L):
            run = 0.0
            for n in range(int(ptr[l]), int(ptr[l + 1])):
                if c[r, n] >= 0:
                    out["present_length"][r, l] += width[n]
                    out["area_above"][r, l] += width[n] * centres[c[r, n]]
                    run = 0.0
                else:
                    run += width[n]
                    out["longest_gap"][r, l] = max(out["longest_gap"][r, l], run)
    return out


def draw_summary(draw_cell, depth_edges, x, y, ptr=None, weights=None):
    """What joint draws are for: per realisation and sequence of ``ptr`` [L + 1] (None: one sequence) of ``draw_cell`` int [R, N]
    (``track(draws=...)``; index on the axis ``depth_edges``, -1: absent), float64 [R, L] on the draws' device,
    ``present_length`` (m): the summed ``sections.section_widths`` of the soundings where the horizon is present,
    ``area_above`` (m^2): sum of width * depth (cell centre) over the present soundings -- the cross-section above the horizon,
    ``longest_gap`` (m): the largest summed width of a run of absent soundings.
    With ``weights`` [N] (for example ``bodies.sounding_areas(plan)``, m^2) in place of the widths and one sequence, ``area_above`` is the
    volume above the surface (and the other two are areas).  Plain torch; ``draw_summary_reference`` states it in numpy loops."""
    c, centres, width, ptr = _summary_arguments(draw_cell, depth_edges, x, y, ptr, weights, "horizons.draw_summary")
    dev = c.device
    w = torch.as_tensor(width).to(dev)
    depth = torch.as_tensor(centres).to(dev)[c.clamp(min=0)]
    here = c >= 0
    R, L = c.shape[0], ptr.size - 1
    out = {k: torch.zeros((R, L), dtype=torch.float64, device=dev) for k in ("present_length", "area_above", "longest_gap")}
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for l in range(L):
        a, b = int(ptr[l]), int(ptr[l + 1])
        if b <= a:
            continue
        h, wl = here[:, a:b], w[None, a:b]
        out["present_length"][:, l] = torch.where(h, wl, zero).sum(dim=1)
        out["area_above"][:, l] = torch.where(h, wl * depth[:, a:b], zero).sum(dim=1)
        gone = torch.cumsum(torch.where(h, zero, wl).expand(R, b - a), dim=1)   # the absent width so far; a run is its growth since the
        base = torch.cummax(torch.where(h, gone, zero), dim=1).values           # last present sounding (the sum never decreases)
        out["longest_gap"][:, l] = (gone - base).max(dim=1).values
    return out


def connected(draw_cell, a, b):
    """The share of the realisations ``draw_cell`` int [R, N] (-1: absent) in which the horizon is present under every sounding from
    ``a`` to ``b`` (both included): the posterior probability of "no gap from a to b", which no product of marginals gives."""
    c = _draw_cells(draw_cell, None, "horizons.connected")
    N = c.shape[1]
    a, b = _args.check_int(a, 0, N - 1, "horizons.connected: a"), _args.check_int(b, 0, N - 1, "horizons.connected: b")
    lo, hi = min(a, b), max(a, b)
    return float((c[:, lo:hi + 1] >= 0).all(dim=1).to(torch.float64).mean())


def percentile_cells(marginal_cells, p):
    """The first cell at which the cumulated marginal over the CELLS (renormalised without the absent state) reaches ``p`` percent:
    int64 [N], and -1 where the cells hold no mass.  ``marginal_cells`` [N, S], torch."""
    m = torch.as_tensor(marginal_cells)
    cum = torch.cumsum(m, dim=1)
    tot = cum[:, -1]
    idx = (cum < (float(p) * 0.01) * tot[:, None]).sum(dim=1).clamp(max=m.shape[1] - 1)
    return torch.where(tot > 0, idx, torch.full_like(idx, -1))


def check_depth_edges(depth_edges):
    """``depth_edges`` as float64 [n + 1], ascending and uniform (the rule has one cell width); returns (edges, dz)."""
    e = np.asarray(depth_edges, dtype=np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0.0):
        raise ValueError("horizons: depth_edges must be at least two finite ascending depths")
    w = np.diff(e)
    dz = (e[-1] - e[0]) / w.size
    if np.any(np.abs(w - dz) > 1e-9 * max(abs(e[-1]), abs(e[0]), dz)):
        raise ValueError("horizons: non-uniform depth cells are not supported (the transition cost depends on cell differences alone)")
    return e, float(dz)


def window(depth_edges, between=None):
    """(lo, hi) of the cells whose centres lie in ``between`` = (d0, d1), d0 <= centre < d1 (None: every cell)."""
    e, _ = check_depth_edges(depth_edges)
    n = e.size - 1
    if between is None:
        return 0, n
    d0, d1 = (float(v) for v in between)
    if not d0 < d1:
        raise ValueError("horizons: between must be (d0, d1) with d0 < d1")
    c = 0.5 * (e[1:] + e[:-1])
    lo, hi = int(np.searchsorted(c, d0, side="left")), int(np.searchsorted(c, d1, side="left"))
    if hi <= lo:
        raise ValueError("horizons: no depth cell has its centre in [%g, %g)" % (d0, d1))
    return lo, hi


def _launch(score, absent_score, ptr, g, d, dz, switch, marginals):
    """gbp_horizon_track on device tensors: score [T, S] fp64, absent_score [T] or None, ptr numpy [L + 1] (checked), g, d numpy [T]."""
    dev = score.device
    total, S = score.shape
    L = ptr.size - 1
    SA = S + (absent_score is not None)
    f64 = dict(dtype=torch.float64, device=dev)
    score = score.contiguous()
    absent_score = None if absent_score is None else absent_score.contiguous()
    t_ptr = torch.as_tensor(ptr, dtype=torch.int64).to(dev)
    t_g, t_d = torch.as_tensor(g, dtype=torch.float64).to(dev), torch.as_tensor(d, dtype=torch.float64).to(dev)
    back = torch.empty((total, S + 1), dtype=torch.int16, device=dev)
    out = dict(cell=torch.empty(total, dtype=torch.int32, device=dev), log_score=torch.empty(L, **f64))
    if marginals:
        out.update(marginal=torch.empty((total, SA), **f64), log_partition=torch.empty(L, **f64), scale=torch.empty(total, **f64))
    _lib.call("gbp_horizon_track", dev, L, t_ptr, total, int(np.diff(ptr).max()) if L else 0, S, float(dz), score, absent_score, t_g, t_d,
              float(switch), back, out["cell"], out["log_score"], out.get("marginal"), out.get("log_partition"), out.get("scale"))
    return out


def _track_arguments(evidence, x, y, surface, absent, slope, switch, floor, ptr, min_distance=1.0):
    """The checks of ``track`` that need no device; returns (ptr, g, d, switch)."""
    if not isinstance(evidence, torch.Tensor) or evidence.ndim != 2:
        raise ValueError("horizons.track: evidence must be a torch tensor [N, n_depth]")
    total = evidence.shape[0]
    if total < 1:
        raise ValueError("horizons.track: no soundings")
    ptr = check_ptr([0, total] if ptr is None else (ptr.cpu().numpy() if isinstance(ptr, torch.Tensor) else ptr), total)
    if not (np.size(x) == np.size(y) == np.size(surface) == total):
        raise ValueError("horizons.track: x, y and surface must hold one entry per sounding (%d)" % total)
    g, d = steps(x, y, surface, slope, min_distance, ptr)
    switch = float(switch)
    if not (np.isfinite(switch) and switch >= 0.0):
        raise ValueError("horizons.track: switch must be >= 0")
    if not 0.0 < float(floor) < 1.0:
        raise ValueError("horizons.track: floor must lie in (0, 1)")
    if absent is not None and tuple(torch.as_tensor(absent).shape) != (total,):
        raise ValueError("horizons.track: absent must hold one weight per sounding")
    return ptr, g, d, switch


def _check_draws(draws, seed, what):
    from . import sections
    return _args.check_int(draws, 0, MAX_DRAWS, "%s: draws" % what), sections._check_seed(seed)


def _track_cells(evidence, absent, ptr, g, d, dz, switch, floor, marginals, draws=0, seed=0, row_key=None):
    """Scores of the (already windowed) evidence and the launch; the outputs are in cells of the window.  With ``draws`` > 0 a second
    launch (``draw``) adds ``draw_state`` int32 [R, sum N] and ``draw_log_score`` [R, L]; with 0 nothing else runs."""
    if evidence.shape[1] > MAX_STATES:
        raise ValueError("horizons.track: %d states, at most %d (choose a window with between=)" % (evidence.shape[1], MAX_STATES))
    if evidence.device.type != "cuda":
        raise _lib.NativeLibraryError("horizons.track runs on the device (gbp_horizon_track); there is no host fallback")
    score, absent_score = evidence_scores(evidence, absent, floor)
    raw = _launch(score, absent_score, ptr, g, d, dz, switch, marginals)
    if draws:
        score = score.contiguous()
        state = draw(ptr, score, absent_score, g, d, dz, switch, draws, seed=seed, row_key=row_key)["draw_state"]
        raw.update(draw_state=state, draw_log_score=draw_log_scores(state, ptr, score, absent_score, g, d, dz, switch))
    return raw


def _finish(raw, S, lo, edges, surface, percentiles):
    """The public entries from the launch's: cells of the window ``lo`` .. ``lo + S - 1`` of the axis ``edges``."""
    dev = raw["cell"].device
    centres = torch.as_tensor(0.5 * (edges[1:] + edges[:-1]), dtype=torch.float64, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    surf = torch.as_tensor(np.asarray(surface, dtype=np.float64).reshape(-1), device=dev)
    c = raw["cell"].long()
    gone = c >= S
    depth = torch.where(gone, nan, centres[(c + lo).clamp(max=centres.numel() - 1)])
    out = dict(cell=torch.where(gone, torch.full_like(raw["cell"], -1), raw["cell"] + lo), depth=depth, elevation=surf - depth,
               log_score=raw["log_score"])
    if "marginal" in raw:
        m = raw["marginal"]
        out["marginal"] = m[:, :S]
        out["absent_probability"] = m[:, S] if m.shape[1] > S else torch.zeros(m.shape[0], dtype=torch.float64, device=dev)
        for p in percentiles:
            i = percentile_cells(m[:, :S], p)
            out[percentile_name(p)] = torch.where(i < 0, nan, centres[(i + lo).clamp(min=0, max=centres.numel() - 1)])
        if "log_partition" in raw:                                             # (a chain's; the survey graph has none)
            out["log_partition"], out["scale"] = raw["log_partition"], raw["scale"]
    if "draw_state" in raw:
        x = raw["draw_state"]
        gone = x >= S
        depth = torch.where(gone, nan, centres[(x.long() + lo).clamp(max=centres.numel() - 1)])
        out.update(draw_cell=torch.where(gone, torch.full_like(x, -1), x + lo), draw_depth=depth, draw_elevation=surf[None, :] - depth,
                   draw_log_score=raw["draw_log_score"])
    return out


def check_percentiles(percentiles):
    ps = tuple(float(p) for p in percentiles)
    if any(not 0.0 < p < 100.0 for p in ps):
        raise ValueError("horizons: percentiles must lie in (0, 100)")
    return ps


def track(evidence, x, y, surface, depth_edges, absent=None, between=None, slope=0.05, switch=4.6, floor=1e-6, marginals=True,
          percentiles=(5, 50, 95), ptr=None, draws=0, seed=0):
    """Track one horizon per sequence through the ``evidence`` [sum N, n_depth] (a torch tensor on the device: non-negative weights on
    the cells of the uniform ``depth_edges`` [n_depth + 1]) of soundings at ``x``, ``y`` on ``surface`` [sum N] (host arrays; m).
    ``absent`` [sum N]: the weight of "no such horizon here" (None: no absent state).  ``between`` = (d0, d1): only the cells with
    d0 <= centre < d1 are states.  ``slope``: the scale of the apparent dip between neighbours, metres of elevation per metre of
    distance -- smaller ties the path more tightly to its neighbours.  ``switch``: the price (nats) of entering or leaving the absent
    state; 4.6 = ln 100.  ``ptr`` [L + 1]: several sequences (lines) in one launch.

    Returns, on the evidence's device: ``cell`` int32 (index on the full axis; -1: absent), ``depth`` (cell centre, NaN: absent),
    ``elevation`` = surface - depth, ``log_score`` [L]; with ``marginals`` also ``marginal`` [sum N, S] over the window's cells,
    ``absent_probability`` [sum N], ``depth_percentile_<p>`` (centre of the first cell at which the cumulated marginal over the cells,
    renormalised without the absent state, reaches p; NaN without mass), ``log_partition`` [L] (the evidence of the chain) and
    ``scale`` [sum N] (s_n, the evidence of sounding n given those before it).

    ``draws`` = R > 0 adds R joint realisations of every sequence's horizon (``draw``), drawn with ``seed`` and the row
    index as the key: ``draw_cell`` int32 [R, sum N] (index on the full axis; -1: absent), ``draw_depth`` and ``draw_elevation``
    [R, sum N] (NaN: absent) and ``draw_log_score`` [R, L] on the scale of ``log_score``, so that ``draw_log_score - log_partition`` is
    a path's log probability.  With ``draws`` = 0 every other output keeps its bits and nothing else is launched."""
    ptr, g, d, switch = _track_arguments(evidence, x, y, surface, absent, slope, switch, floor, ptr)
    draws, seed = _check_draws(draws, seed, "horizons.track")
    percentiles = check_percentiles(percentiles)
    edges, dz = check_depth_edges(depth_edges)
    if evidence.shape[1] != edges.size - 1:
        raise ValueError("horizons.track: evidence has %d depth cells, depth_edges %d" % (evidence.shape[1], edges.size - 1))
    lo, hi = window(edges, between)
    raw = _track_cells(evidence[:, lo:hi], absent, ptr, g, d, dz, switch, floor, marginals, draws, seed)
    return _finish(raw, hi - lo, lo, edges, surface, percentiles)


def _stack(parts, between, percentiles):
    """Per-horizon results stacked [H, N]; the marginals keep their own widths as ``marginal_<h>``."""
    out = {}
    for k in parts[0]:
        if k == "marginal":
            for h, p in enumerate(parts):
                out["marginal_%d" % h] = p[k]
        elif k in ("log_score", "log_partition"):
            out[k] = torch.cat([p[k].reshape(1) for p in parts])
        elif k == "draw_log_score":
            out[k] = torch.stack([p[k][:, 0] for p in parts])                  # [H, R]: every horizon is one sequence
        else:
            out[k] = torch.stack([p[k] for p in parts])
    if between is not None:
        out["between"] = np.asarray(between, dtype=np.float64).reshape(-1, 2)
    return out


def _split(res, h, N):
    """Sequence ``h`` of a launch of sequences of N soundings each."""
    cut = {"log_score": lambda v: v[h:h + 1], "log_partition": lambda v: v[h:h + 1], "draw_log_score": lambda v: v[:, h:h + 1],
           "draw_state": lambda v: v[:, h * N:(h + 1) * N]}
    return {k: cut.get(k, lambda v: v[h * N:(h + 1) * N])(v) for k, v in res.items()}


def _read(path_or_products, container):
    """(interface_probability, interface_depth_edges, x, y, surface) as numpy from products / a products file / a container."""
    from . import hdf, line_products as lp
    prob = edges = arrays = None
    src = path_or_products
    if isinstance(src, dict):
        prob, edges = src.get("interface_probability"), src.get("interface_depth_edges", src.get("depth_edges"))
    elif str(src).endswith(".npz") and not str(src).endswith(".results.npz"):
        with np.load(src) as f:
            prob = f["interface_probability"] if "interface_probability" in f else None
            edges = f["interface_depth_edges"] if "interface_depth_edges" in f else (f["depth_edges"] if "depth_edges" in f else None)
    else:
        container = src if container is None else container
    if container is not None:
        arrays, _ = hdf.load_results(container)
    if prob is None and arrays is not None:
        ic, ix, iz = (lp._key(arrays, lp.INTERFACES + k) for k in ("/values/data", "/mesh/x/edges/data", "/mesh/y/edges/data"))
        if ic is not None and ix is not None and iz is not None and np.ndim(ic) == 2:
            prob, edges = lp.interface_pdf(ic, ix, iz).numpy(), np.asarray(iz, dtype=np.float64)
    if prob is None or edges is None:
        raise ValueError("horizons.from_products: no interface_probability on interface_depth_edges in %s" % (
            "the products" if isinstance(src, dict) else src))
    x = y = s = None
    if arrays is not None:
        x, y = lp._key(arrays, "/data/x/data", "/data/x"), lp._key(arrays, "/data/y/data", "/data/y")
        s = lp._key(arrays, "/data/elevation/data", "/data/elevation")
    return np.asarray(prob, dtype=np.float64), np.asarray(edges, dtype=np.float64), x, y, s


def from_products(path_or_products, between, container=None, x=None, y=None, surface=None, slope=0.05, switch=4.6, floor=1e-6,
                  marginals=True, percentiles=(5, 50, 95), absent=False, device=None, draws=0, seed=0):
    """One horizon per window of ``between`` = [(d0, d1), ...] through the ``interface_probability`` [N, n_depth] on
    ``interface_depth_edges`` of a results container (``<line>.h5``), of line products (a dict of ``line_products.from_results``) or
    of saved line products (``<line>.products.npz``); x, y and the surface elevation come from the ``container`` (with a container
    path as the first argument: that one) unless given.  ``absent`` = True adds the absent state with the weight of the probability
    mass outside the window.  The windows with equal cell counts run in one launch.  Returns the entries of ``track`` stacked
    [H, N] (``log_score``, ``log_partition`` [H]), ``marginal_<h>`` [N, S_h] and ``between`` [H, 2], on ``device`` (default cuda:0).
    ``draws`` = R > 0 adds ``draw_cell``, ``draw_depth``, ``draw_elevation`` [H, R, N] and ``draw_log_score`` [H, R] (``track``); the key
    of sounding n under window h is n + h N, so two horizons of one sounding never share a uniform, and a window keeps its draws
    whichever other windows are asked for before it."""
    prob, edges, cx, cy, cs = _read(path_or_products, container)
    x, y, surface = (cx if x is None else x), (cy if y is None else y), (cs if surface is None else surface)
    if x is None or y is None or surface is None:
        raise ValueError("horizons.from_products: x, y and surface are needed (give them, or a container that holds them)")
    wins = [tuple(float(v) for v in w) for w in np.asarray(between, dtype=np.float64).reshape(-1, 2)]
    if not wins:
        raise ValueError("horizons.from_products: at least one window (d0, d1) is needed")
    edges, dz = check_depth_edges(edges)
    percentiles = check_percentiles(percentiles)
    draws, seed = _check_draws(draws, seed, "horizons.from_products")
    N = prob.shape[0]
    if prob.ndim != 2 or prob.shape[1] != edges.size - 1:
        raise ValueError("horizons.from_products: interface_probability %r does not match its %d depth cells" % (prob.shape, edges.size - 1))
    ranges = [window(edges, w) for w in wins]
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    e = torch.as_tensor(np.nan_to_num(prob, nan=0.0)).to(dev) if dev.type == "cuda" else torch.as_tensor(np.nan_to_num(prob, nan=0.0))
    parts = [None] * len(wins)
    for S in sorted({hi - lo for lo, hi in ranges}):
        hs = [h for h, (lo, hi) in enumerate(ranges) if hi - lo == S]
        ev = torch.cat([e[:, ranges[h][0]:ranges[h][1]] for h in hs])
        ab = torch.cat([e.sum(1) - e[:, ranges[h][0]:ranges[h][1]].sum(1) for h in hs]).clamp(min=0.0) if absent else None
        tile = lambda a: np.tile(np.asarray(a, dtype=np.float64).reshape(-1), len(hs))       # noqa: E731
        ptr, g, d, sw = _track_arguments(ev, tile(x), tile(y), tile(surface), ab, slope, switch, floor, np.arange(len(hs) + 1) * N)
        key = np.concatenate([np.arange(N, dtype=np.int64) + h * N for h in hs]) if draws else None
        raw = _track_cells(ev, ab, ptr, g, d, dz, sw, floor, marginals, draws, seed, key)
        for i, h in enumerate(hs):
            parts[h] = _finish(_split(raw, i, N), S, ranges[h][0], edges, surface, percentiles)
    return _stack(parts, wins, percentiles)


def from_chains(dc_or_dict, x, y, surface, slope=0.05, switch=4.6, floor=1e-6, marginals=True, percentiles=(5, 50, 95)):
    """One horizon per threshold of a sampler's ``first_above`` / ``first_below`` (``rjmcmc_gpu.DeviceChains``, or a dict of its
    ``first_hist`` [N, T, n_depth], ``first_none`` [N, T] and ``depth_bin_width``): the sampled posterior of the depth to the first
    layer beyond the threshold is the evidence and the count of samples without such a layer the weight of the absent state.  The
    chains are the soundings of ONE line, at ``x``, ``y`` on ``surface`` [N].  All T horizons run in one launch; the result is that of
    ``from_products``, [T, N]."""
    from . import unit_posteriors
    _, fh, fnone, _, _, _, _, dbw = unit_posteriors._arrays(dc_or_dict)
    if fh is None or fnone is None or dbw is None:
        raise ValueError("horizons.from_chains: the sampler holds no first_hist / first_none (DeviceChains(first_above=..., first_below=...))")
    fh, fnone = torch.as_tensor(fh), torch.as_tensor(fnone)
    if fh.ndim != 3 or tuple(fnone.shape) != tuple(fh.shape[:2]):
        raise ValueError("horizons.from_chains: first_hist must be [N, T, n_depth] and first_none [N, T]")
    N, T, nz = fh.shape
    percentiles = check_percentiles(percentiles)
    edges = np.arange(nz + 1, dtype=np.float64) * float(dbw)
    ev = fh.permute(1, 0, 2).reshape(T * N, nz).to(torch.float64)
    ab = fnone.to(fh.device).permute(1, 0).reshape(T * N).to(torch.float64)
    tile = lambda a: np.tile(np.asarray(a, dtype=np.float64).reshape(-1), T)                  # noqa: E731
    ptr, g, d, sw = _track_arguments(ev, tile(x), tile(y), tile(surface), ab, slope, switch, floor, np.arange(T + 1) * N)
    raw = _track_cells(ev, ab, ptr, g, d, float(dbw), sw, floor, marginals)
    return _stack([_finish(_split(raw, t, N), nz, 0, edges, surface, percentiles) for t in range(T)], None, percentiles)


def as_intervals(top, bottom):
    """{"kind": "horizons", "top": ..., "bottom": ...} for ``line_products.from_results(intervals=...)`` from two picks: results of
    ``track`` (their ``depth``) or depth arrays [N]; NaN where a pick is absent, which gives that sounding no unit."""
    def depth(p):
        v = p["depth"] if isinstance(p, dict) else p
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        return np.asarray(v, dtype=np.float64)
    t, b = depth(top), depth(bottom)
    if t.shape != b.shape or t.ndim != 1:
        raise ValueError("horizons.as_intervals: top and bottom must both be [N]")
    return {"kind": "horizons", "top": t, "bottom": b}


# ---- horizon pairs: the top and the base of one unit, tracked jointly and ordered ---------------------------------------

MAX_UNIT_STATES = 96
UNIT_SUFFIX = ".unit.npz"


def _check_unit(ptr, score_top, score_base, g, d, dz, switch, min_cells, thickness_score, absent_score, what):
    """The checks ``unit_reference`` and the launch share, on shapes and host values alone (the scores numpy or torch, any device);
    returns ptr (int64 numpy), g, d (float64 numpy), dz, switch and min_cells."""
    if getattr(score_top, "ndim", 0) != 2 or score_top.shape[1] < 1 or tuple(score_base.shape) != tuple(score_top.shape):
        raise ValueError("%s: score_top and score_base must both be [N, S] with S >= 1" % what)
    total, S = score_top.shape
    ptr = check_ptr(ptr, total)
    g, d = np.asarray(_args.host(g), dtype=np.float64).reshape(-1), np.asarray(_args.host(d), dtype=np.float64).reshape(-1)
    if g.size != total or d.size != total:
        raise ValueError("%s: g and d must hold one entry per sounding" % what)
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(d))):
        raise ValueError("%s: g and d must be finite" % what)
    min_cells = _args.check_int(min_cells, 0, S - 1, "%s: min_cells (S = %d)" % (what, S))
    if thickness_score is not None and tuple(thickness_score.shape) != (S,):
        raise ValueError("%s: thickness_score must hold one entry per thickness b - a = 0 .. S - 1 (%d)" % (what, S))
    if absent_score is not None and tuple(absent_score.shape) != (total,):
        raise ValueError("%s: absent_score must hold one entry per sounding" % what)
    dz, switch = float(dz), float(switch)
    if not (np.isfinite(dz) and dz > 0.0):
        raise ValueError("%s: dz must be positive" % what)
    if not (np.isfinite(switch) and switch >= 0.0):
        raise ValueError("%s: switch must be >= 0" % what)
    return ptr, g, d, dz, switch, min_cells


def unit_reference(ptr, score_top, score_base, g, d, dz, switch, min_cells=1, thickness_score=None, absent_score=None, marginals=True,
                   dtype=np.float64):
    """The rule of ``unit`` in numpy, evaluated in ``dtype`` (fp64: what the device is held to; np.longdouble: the yardstick of the
    rule's own rounding): the top and the base of one unit as ONE Markov chain, so that the base never lies above the top.  ``ptr``,
    ``g``, ``d`` (``steps``), ``dz`` and ``switch`` as ``track_reference`` takes them; ``score_top``, ``score_base`` [sum N, S] on one
    shared window of S cells; ``thickness_score`` [S] or None, indexed by b - a and shared by all soundings; ``absent_score`` [sum N]
    or None.

    States: the pairs (a, b) of cells, a the top and b the base, valid when b - a >= ``min_cells`` (0 .. S - 1; 0 allows a == b, a
    unit pinched to nothing), and optionally "absent", which comes last in every order.  Node score s[n, a, b] = (score_top[n, a] +
    score_base[n, b]) + thickness_score[b - a] -- without ``thickness_score`` the term is left out --; invalid pairs hold -inf (weight
    0 in the linear domain).
    Step n -> n + 1: T_n[k] = g[n] |d[n] - k dz|, ``track``'s table; pair -> pair costs T_n[a' - a] + T_n[b' - b], applied in two
    passes whose order defines the bits and the ties: pass 1 M1[a', b] = max over a ascending of V[a, b] - T[a' - a]; pass 2
    M2[a', b'] = max over b ascending of M1[a', b] - T[b' - b]; then the candidate V[absent] - switch; every maximum keeps the first
    (strict > replaces).  V'[a', b'] = s[n + 1, a', b'] + M2 for valid pairs.  V'[absent] = absent_score[n + 1] + the first maximum of
    V[a, b] - switch over the valid pairs in row-major order (a, then b ascending), which V[absent] replaces on strict >.  The path
    ends at the first maximum of the last V in row-major order, then absent; the walk back follows pass 2's argument, then pass 1's.
    Marginals: the same two passes as sums, scaled forward-backward in the linear domain laid out as in ``track_reference``: w =
    exp(s), K = exp(-T), ks = exp(-switch); the sums run a ascending, then b ascending (acc = acc + alpha K); alpha is normalised by
    its sum s_n; backward the passes run over a', then b', with the mirrored table.

    Returns ``cell_top``, ``cell_base`` int32 [sum N] (both S: absent), ``log_score`` [L], and with ``marginals``
    ``marginal_top``, ``marginal_base`` [sum N, S] (gamma summed over the other cell), ``marginal_thickness`` [sum N, S] (indexed by
    b - a), ``marginal_absent`` [sum N], ``log_partition`` [L] and ``scale`` [sum N] (s_n).  The full pair marginal is not returned."""
    what = "horizons.unit_reference"
    ft = np.dtype(dtype).type
    score_top, score_base = np.asarray(score_top, dtype=np.float64), np.asarray(score_base, dtype=np.float64)
    thickness_score = None if thickness_score is None else np.asarray(thickness_score, dtype=np.float64)
    has_absent = absent_score is not None
    absent_score = np.asarray(absent_score, dtype=np.float64).reshape(-1) if has_absent else None
    ptr, g, d, dz, switch, mc = _check_unit(ptr, score_top, score_base, g, d, dz, switch, min_cells, thickness_score, absent_score, what)
    if not (np.all(np.isfinite(score_top)) and np.all(np.isfinite(score_base)) and (thickness_score is None or np.all(np.isfinite(thickness_score)))
            and (not has_absent or np.all(np.isfinite(absent_score)))):
        raise ValueError("%s: the scores must be finite" % what)
    total, S = score_top.shape
    st, sb, g, d = score_top.astype(ft), score_base.astype(ft), g.astype(ft), d.astype(ft)
    absent_score = absent_score.astype(ft) if has_absent else None
    dz, switch = ft(dz), ft(switch)
    L, SS = ptr.size - 1, S * S
    kf = np.arange(-(S - 1), S).astype(ft)                                   # k = c' - c at index k + S - 1
    diff = np.arange(S)[None, :] - np.arange(S)[:, None]                     # b - a at [a, b]
    valid = diff >= mc
    ts = None if thickness_score is None else thickness_score.astype(ft)[np.maximum(diff, 0)]
    ninf = ft(-np.inf)

    def node(r):
        s = st[r][:, None] + sb[r][None, :]
        return np.where(valid, s if ts is None else s + ts, ninf)

    cell_top, cell_base, log_score = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32), np.zeros(L, dtype=ft)
    out = dict(cell_top=cell_top, cell_base=cell_base, log_score=log_score)
    if marginals:
        m_top, m_base, m_thick = (np.zeros((total, S), dtype=ft) for _ in range(3))
        m_absent, log_partition, scale = np.zeros(total, dtype=ft), np.zeros(L, dtype=ft), np.zeros(total, dtype=ft)
        out.update(marginal_top=m_top, marginal_base=m_base, marginal_thickness=m_thick, marginal_absent=m_absent,
                   log_partition=log_partition, scale=scale)
    # for a fixed c the costs of all c' are the slice [S - 1 - c, 2 S - 1 - c) of the table; for a fixed c' those of all c the slice
    # [c', c' + S) reversed (``track_reference``)
    for l in range(L):
        r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
        # ---- Viterbi
        V = node(r0)
        Va = absent_score[r0] if has_absent else ninf
        back1, back2 = np.zeros((N, S, S), dtype=np.int64), np.zeros((N, S, S), dtype=np.int64)
        back_absent = np.zeros(N, dtype=np.int64)
        for n in range(N - 1):
            T = g[r0 + n] * np.abs(d[r0 + n] - kf * dz)
            m1, a1 = np.full((S, S), ninf, dtype=ft), np.zeros((S, S), dtype=np.int64)            # [a', b]
            for a in range(S):
                cand = V[a][None, :] - T[S - 1 - a:2 * S - 1 - a][:, None]
                repl = cand > m1                                             # strict: the first maximum stays
                m1, a1 = np.where(repl, cand, m1), np.where(repl, a, a1)
            m2, a2 = np.full((S, S), ninf, dtype=ft), np.zeros((S, S), dtype=np.int64)            # [a', b']
            for b in range(S):
                cand = m1[:, b][:, None] - T[S - 1 - b:2 * S - 1 - b][None, :]
                repl = cand > m2
                m2, a2 = np.where(repl, cand, m2), np.where(repl, b, a2)
            if has_absent:
                via = Va - switch
                repl = via > m2
                m2, a2 = np.where(repl, via, m2), np.where(repl, S, a2)
                flat = (V - switch).reshape(-1)                              # (-inf where the pair is invalid: never the maximum)
                a_arg = first_max(flat)
                a_m = flat[a_arg]
                if Va > a_m:
                    a_arg, a_m = SS, Va
                Va = absent_score[r0 + n + 1] + a_m
                back_absent[n + 1] = a_arg
            V = np.where(valid, node(r0 + n + 1) + m2, ninf)
            back1[n + 1], back2[n + 1] = a1, a2
        flat = V.reshape(-1)
        cur = first_max(flat)
        log_score[l] = flat[cur]
        if has_absent and Va > flat[cur]:
            cur, log_score[l] = SS, Va
        for n in range(N - 1, -1, -1):
            a, b = divmod(cur, S) if cur < SS else (S, S)
            cell_top[r0 + n], cell_base[r0 + n] = a, b
            if n > 0:
                if cur == SS:
                    cur = int(back_absent[n])
                else:
                    pb = int(back2[n, a, b])
                    cur = SS if pb == S else int(back1[n, a, pb]) * S + pb
        if not marginals:
            continue
        # ---- scaled forward-backward
        ks = np.exp(-switch)
        zero = ft(0.0)
        w = np.exp(np.stack([node(r0 + n) for n in range(N)]))                 # [N, S, S], 0 where the pair is invalid
        wa = np.exp(absent_score[r0:r0 + N]) if has_absent else np.zeros(N, dtype=ft)
        alpha, alpha_a, s = np.zeros((N, S, S), dtype=ft), np.zeros(N, dtype=ft), np.zeros(N, dtype=ft)
        s[0] = w[0].sum() + (wa[0] if has_absent else zero)
        alpha[0], alpha_a[0] = w[0] / s[0], wa[0] / s[0]
        Ks = []
        for n in range(N - 1):
            K = np.exp(-(g[r0 + n] * np.abs(d[r0 + n] - kf * dz)))
            Ks.append(K)
            p1 = np.zeros((S, S), dtype=ft)                                  # [a', b]
            for a in range(S):                                               # a ascending
                p1 = p1 + alpha[n, a][None, :] * K[S - 1 - a:2 * S - 1 - a][:, None]
            p2 = np.zeros((S, S), dtype=ft)                                  # [a', b']
            for b in range(S):                                               # b ascending
                p2 = p2 + p1[:, b][:, None] * K[S - 1 - b:2 * S - 1 - b][None, :]
            ua = zero
            if has_absent:
                p2 = p2 + alpha_a[n] * ks
                ua = wa[n + 1] * (np.cumsum((alpha[n] * ks).reshape(-1))[-1] + alpha_a[n])
            u = w[n + 1] * p2
            s[n + 1] = u.sum() + ua
            alpha[n + 1], alpha_a[n + 1] = u / s[n + 1], ua / s[n + 1]
        beta, beta_a = np.ones((S, S), dtype=ft), ft(1.0)
        for n in range(N - 1, -1, -1):
            if n < N - 1:
                K = Ks[n]
                u, ua = w[n + 1] * beta, wa[n + 1] * beta_a
                q1 = np.zeros((S, S), dtype=ft)                              # [a, b']
                for c in range(S):                                           # a' ascending
                    q1 = q1 + K[c:c + S][::-1][:, None] * u[c][None, :]
                q2 = np.zeros((S, S), dtype=ft)                              # [a, b]
                for c in range(S):                                           # b' ascending
                    q2 = q2 + q1[:, c][:, None] * K[c:c + S][::-1][None, :]
                if has_absent:
                    q2 = q2 + ks * ua
                    beta_a = (np.cumsum((ks * u).reshape(-1))[-1] + ua) / s[n + 1]
                beta = q2 / s[n + 1]
            gm = alpha[n] * beta                                             # (0 where the pair is invalid: alpha is)
            gm_a = alpha_a[n] * beta_a if has_absent else zero
            tot = gm.sum() + gm_a
            gamma = gm / tot
            m_top[r0 + n], m_base[r0 + n] = gamma.sum(axis=1), gamma.sum(axis=0)
            m_thick[r0 + n] = [np.trace(gamma, offset=k) for k in range(S)]
            m_absent[r0 + n] = gm_a / tot
        scale[r0:r0 + N] = s
        log_partition[l] = np.cumsum(np.log(s))[-1]
    return out


def unit_bytes(total, S, marginals=True):
    """The bytes of the workspaces a launch of ``total`` soundings and S cells holds: the back-pointers of the two passes, uint8
    [2, total, S, S], those of the absent state, int32 [total], and with ``marginals`` alpha, float64 [total, S S + 1]."""
    total, S = int(total), int(S)
    return total * (2 * S * S + 4) + (total * (S * S + 1) * 8 if marginals else 0)


def _unit_launch(score_top, score_base, thickness_score, absent_score, ptr, g, d, dz, switch, min_cells, marginals, budget_bytes=4 << 30):
    """gbp_horizon_unit_track on device tensors (float64, score_top and score_base [T, S], thickness_score [S] or None, absent_score [T]
    or None), ptr numpy [L + 1], g, d numpy [T].  The launch is split by whole sequences so that the workspaces of a part
    (``unit_bytes``) stay under ``budget_bytes``; the parts are independent, so the split changes no bit."""
    entry, what = "gbp_horizon_unit_track", "horizons.unit"
    for a in (score_top, score_base, thickness_score, absent_score):
        if a is not None and not isinstance(a, torch.Tensor):
            raise TypeError("%s: the scores are torch tensors (%s runs on the device)" % (what, entry))
    ptr, g, d, dz, switch, mc = _check_unit(ptr, score_top, score_base, g, d, dz, switch, min_cells, thickness_score, absent_score, what)
    total, S = score_top.shape
    if S > MAX_UNIT_STATES:
        raise ValueError("%s: %d states, at most %d (choose a narrower window with between=, or coarsen=)" % (what, S, MAX_UNIT_STATES))
    budget_bytes = _args.check_int(budget_bytes, 1, 2 ** 62, "%s: budget_bytes" % what)
    given = tuple(a for a in (score_top, score_base, thickness_score, absent_score) if a is not None)
    if any(a.dtype != torch.float64 for a in given):
        raise TypeError("%s: the scores are float64" % what)
    if thickness_score is not None and not bool(torch.isfinite(thickness_score).all()):      # (S values: the one score array small enough to check)
        raise ValueError("%s: thickness_score must be finite" % what)
    L = ptr.size - 1
    parts, a = [], 0                                                          # [l0, l1) of whole sequences under the budget
    while a < L:
        b = a + 1
        if unit_bytes(ptr[b] - ptr[a], S, marginals) > budget_bytes:
            raise ValueError("%s: the workspaces of one sequence of %d soundings and %d cells take %d bytes, more than budget_bytes = %d; "
                             "choose a narrower window with between=, or coarsen=" % (what, ptr[b] - ptr[a], S, unit_bytes(ptr[b] - ptr[a], S, marginals),
                                                                                     budget_bytes))
        while b < L and unit_bytes(ptr[b + 1] - ptr[a], S, marginals) <= budget_bytes:
            b += 1
        parts.append((a, b))
        a = b
    _args.on_device(given, "horizons", "unit", entry)
    dev = score_top.device
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    score_top, score_base = score_top.contiguous(), score_base.contiguous()
    thickness_score = None if thickness_score is None else thickness_score.contiguous()
    absent_score = None if absent_score is None else absent_score.contiguous()
    t_g, t_d = torch.as_tensor(g).to(dev), torch.as_tensor(d).to(dev)
    out = dict(cell_top=torch.empty(total, **i32), cell_base=torch.empty(total, **i32), log_score=torch.empty(L, **f64))
    if marginals:
        out.update(marginal_top=torch.empty((total, S), **f64), marginal_base=torch.empty((total, S), **f64),
                   marginal_thickness=torch.empty((total, S), **f64), marginal_absent=torch.empty(total, **f64),
                   log_partition=torch.empty(L, **f64), scale=torch.empty(total, **f64))
    rows = ("cell_top", "cell_base", "marginal_top", "marginal_base", "marginal_thickness", "marginal_absent", "scale")
    for l0, l1 in parts:
        r0, r1 = int(ptr[l0]), int(ptr[l1])
        n = r1 - r0
        cut = {k: (v[r0:r1] if k in rows else v[l0:l1]) for k, v in out.items()}
        back = torch.empty((2, n, S, S), dtype=torch.uint8, device=dev)
        back_absent = None if absent_score is None else torch.empty(n, **i32)
        alpha = torch.empty((n, S * S + 1), **f64) if marginals else None
        _lib.call(entry, dev, l1 - l0, torch.as_tensor(ptr[l0:l1 + 1] - r0).to(dev), n, int(np.diff(ptr[l0:l1 + 1]).max()), S, mc, dz,
                  score_top[r0:r1], score_base[r0:r1], thickness_score, None if absent_score is None else absent_score[r0:r1], t_g[r0:r1],
                  t_d[r0:r1], switch, back, back_absent, cut["cell_top"], cut["cell_base"], cut["log_score"], alpha, cut.get("marginal_top"),
                  cut.get("marginal_base"), cut.get("marginal_thickness"), cut.get("marginal_absent"), cut.get("log_partition"), cut.get("scale"))
    return out


def _pair(value):
    """``value`` as (top, base): one object serves both horizons."""
    return tuple(value) if isinstance(value, (tuple, list)) and len(value) == 2 else (value, value)


def unit(evidence_top, evidence_base, x, y, surface, depth_edges, between=None, top_between=None, base_between=None, min_thickness=None,
         coarsen=1, absent=None, thickness_score=None, slope=0.05, switch=4.6, floor=1e-6, marginals=True, percentiles=(5, 50, 95), ptr=None,
         budget_bytes=4 << 30):
    """Track the top and the base of one unit per sequence jointly, the base never less than ``min_thickness`` below the top
    (gbp_horizon_unit_track; ``unit_reference`` states the rule).  ``evidence_top``, ``evidence_base`` [sum N, n_depth]:
    torch tensors on the device, non-negative weights on the cells of the uniform ``depth_edges`` (``evidence_base`` None: the same
    evidence for both); ``x``, ``y``, ``surface`` [sum N], ``slope``, ``switch``, ``floor``, ``ptr`` as ``track`` takes them.
    ``between`` = (d0, d1): the window the two horizons share.  ``top_between`` / ``base_between`` = (d0, d1): the evidence of that
    horizon is set to zero in the cells whose centres lie outside it, before anything else.  ``coarsen`` = C: groups of C cells of the
    window are summed on the device before scoring, and a trailing partial group is dropped from the window; the states are the
    S <= 96 groups.  ``min_thickness`` (m) becomes min_cells = ceil(min_thickness / (C dz)), 0 allowing a unit pinched to nothing (None:
    one cell; 0 where the window is a single cell, S = 1, which has no other pair).  Each horizon's scores are ``evidence_scores`` of its evidence; ``absent``: one weight array [sum N] or a pair (top,
    base) -- the absent state's score is the sum of the two horizons' absent scores (None: no absent state).  ``thickness_score`` [S]:
    an extra score of the thickness in cells, b - a.  The launch is split by whole sequences under ``budget_bytes`` of workspaces
    (``unit_bytes``), which changes no bit; one sequence beyond it is a ValueError.  There is no host fallback.

    Returns on the evidence's device ``top_cell``, ``base_cell`` int32 (on the full axis: the cell that holds the centre of the
    group, lo + C k + C // 2; -1: absent), ``top_depth``, ``base_depth`` (the group's centre; NaN: absent), ``top_elevation``,
    ``base_elevation``, ``thickness`` (m; NaN: absent), ``log_score`` [L]; with ``marginals`` also ``top_marginal``, ``base_marginal``
    [sum N, S] over the groups, ``thickness_marginal`` [sum N, S] over b - a, ``absent_probability``, ``pinched_probability`` (the
    mass of thickness 0; only with min_cells = 0), ``thickness_mean`` (m, given that the unit is present; NaN without mass),
    ``thickness_percentile_<p>``, ``top_depth_percentile_<p>``, ``base_depth_percentile_<p>`` (``percentile_cells``), ``log_partition``
    [L] and ``scale``; and ``cell_depth_edges`` [S + 1], the edges of the groups."""
    what = "horizons.unit"
    evidence_base = evidence_top if evidence_base is None else evidence_base
    if not isinstance(evidence_base, torch.Tensor) or not isinstance(evidence_top, torch.Tensor) or evidence_base.shape != evidence_top.shape:
        raise ValueError("%s: evidence_top and evidence_base must be torch tensors of one shape [N, n_depth]" % what)
    a_top, a_base = _pair(absent) if absent is not None else (None, None)
    ptr, g, d, switch = _track_arguments(evidence_top, x, y, surface, a_top, slope, switch, floor, ptr)
    if a_base is not None and tuple(torch.as_tensor(a_base).shape) != (evidence_top.shape[0],):
        raise ValueError("%s: absent must hold one weight per sounding" % what)
    percentiles = check_percentiles(percentiles)
    edges, dz = check_depth_edges(depth_edges)
    if evidence_top.shape[1] != edges.size - 1:
        raise ValueError("%s: the evidence has %d depth cells, depth_edges %d" % (what, evidence_top.shape[1], edges.size - 1))
    C = _args.check_int(coarsen, 1, edges.size - 1, "%s: coarsen" % what)
    lo, hi = window(edges, between)
    S = (hi - lo) // C
    if S < 1:
        raise ValueError("%s: the window holds %d cells, fewer than coarsen = %d" % (what, hi - lo, C))
    hi = lo + S * C
    if S > MAX_UNIT_STATES:
        raise ValueError("%s: %d states, at most %d (choose a narrower window with between=, or coarsen=)" % (what, S, MAX_UNIT_STATES))
    if min_thickness is None:
        mc = 1 if S > 1 else 0
    else:
        min_thickness = float(min_thickness)
        if not (np.isfinite(min_thickness) and min_thickness >= 0.0):
            raise ValueError("%s: min_thickness must be >= 0" % what)
        mc = int(np.ceil(min_thickness / (C * dz) - 1e-9))
    if mc > S - 1:
        raise ValueError("%s: min_thickness is %d cells of %g m, the window holds %d (at most %d)" % (what, mc, C * dz, S, S - 1))
    if thickness_score is not None and tuple(torch.as_tensor(thickness_score).shape) != (S,):
        raise ValueError("%s: thickness_score must hold one entry per thickness b - a = 0 .. S - 1 (%d)" % (what, S))
    if evidence_top.device.type != "cuda" or evidence_base.device.type != "cuda":
        raise _lib.NativeLibraryError("%s runs on the device (gbp_horizon_unit_track); there is no host fallback" % what)
    dev = evidence_top.device
    scores = []
    for ev, sub, ab in ((evidence_top, top_between, a_top), (evidence_base, base_between, a_base)):
        ev = ev.to(torch.float64)
        if sub is not None:
            s0, s1 = window(edges, sub)
            keep = torch.zeros(edges.size - 1, dtype=torch.bool, device=dev)
            keep[s0:s1] = True
            ev = torch.where(keep[None, :], ev, torch.zeros((), dtype=torch.float64, device=dev))
        ev = ev[:, lo:hi].reshape(ev.shape[0], S, C).sum(dim=2)
        scores.append(evidence_scores(ev, ab, floor))
    (score_top, ab_top), (score_base, ab_base) = scores
    absent_score = None if ab_top is None else ab_top + ab_base
    t_thick = None if thickness_score is None else torch.as_tensor(thickness_score, dtype=torch.float64).to(dev)
    raw = _unit_launch(score_top, score_base, t_thick, absent_score, ptr, g, d, C * dz, switch, mc, marginals, budget_bytes)
    # the public entries: groups of the window lo .. hi of the axis
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    cell_edges = edges[lo] + C * dz * np.arange(S + 1)
    centres = torch.as_tensor(0.5 * (cell_edges[1:] + cell_edges[:-1]), dtype=torch.float64, device=dev)
    surf = torch.as_tensor(np.asarray(surface, dtype=np.float64).reshape(-1), device=dev)
    ct, cb = raw["cell_top"].long(), raw["cell_base"].long()
    gone = ct >= S
    full = lambda c: torch.where(gone, torch.full_like(c, -1), lo + C * c + C // 2).to(torch.int32)      # noqa: E731
    depth = lambda c: torch.where(gone, nan, centres[c.clamp(max=S - 1)])                              # noqa: E731
    out = dict(top_cell=full(ct), base_cell=full(cb), top_depth=depth(ct), base_depth=depth(cb), log_score=raw["log_score"])
    out.update(top_elevation=surf - out["top_depth"], base_elevation=surf - out["base_depth"],
               thickness=torch.where(gone, nan, (cb - ct).to(torch.float64) * (C * dz)), cell_depth_edges=cell_edges, min_cells=mc)
    if marginals:
        mt, mb, mk = raw["marginal_top"], raw["marginal_base"], raw["marginal_thickness"]
        out.update(top_marginal=mt, base_marginal=mb, thickness_marginal=mk, absent_probability=raw["marginal_absent"])
        if mc == 0:
            out["pinched_probability"] = mk[:, 0]
        width = torch.arange(S, dtype=torch.float64, device=dev) * (C * dz)
        mass = mk.sum(dim=1)
        out["thickness_mean"] = torch.where(mass > 0, (mk * width[None, :]).sum(dim=1) / torch.where(mass > 0, mass, torch.ones_like(mass)), nan)
        for p in percentiles:
            for name, m, value in (("thickness", mk, width), ("top_depth", mt, centres), ("base_depth", mb, centres)):
                i = percentile_cells(m, p)
                out["%s_percentile_%g" % (name, p)] = torch.where(i < 0, nan, value[i.clamp(min=0)])
        out["log_partition"], out["scale"] = raw["log_partition"], raw["scale"]
    return out


def unit_from_products(path_or_products, between, container=None, x=None, y=None, surface=None, absent=False, device=None, **kwargs):
    """``unit`` on the ``interface_probability`` of a results container, of line products or of saved line products (what
    ``from_products`` reads, by the same ``_read``), as the evidence of both horizons in the ONE window ``between`` = (d0, d1); x, y
    and the surface come from the container unless given.  ``absent`` = True adds the absent state with the weight of the probability
    mass outside the window for each horizon.  The other arguments are ``unit``'s; the result is ``unit``'s, on ``device`` (default
    cuda:0)."""
    what = "horizons.unit_from_products"
    prob, edges, cx, cy, cs = _read(path_or_products, container)
    x, y, surface = (cx if x is None else x), (cy if y is None else y), (cs if surface is None else surface)
    if x is None or y is None or surface is None:
        raise ValueError("%s: x, y and surface are needed (give them, or a container that holds them)" % what)
    win = np.asarray(between, dtype=np.float64).reshape(-1)
    if win.size != 2:
        raise ValueError("%s: between must be one window (d0, d1)" % what)
    edges, _ = check_depth_edges(edges)
    if prob.ndim != 2 or prob.shape[1] != edges.size - 1:
        raise ValueError("%s: interface_probability %r does not match its %d depth cells" % (what, prob.shape, edges.size - 1))
    lo, hi = window(edges, tuple(win))
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    e = torch.as_tensor(np.nan_to_num(prob, nan=0.0))
    e = e.to(dev) if dev.type == "cuda" else e
    ab = (e.sum(1) - e[:, lo:hi].sum(1)).clamp(min=0.0) if absent else None
    return unit(e, None, x, y, surface, edges, between=tuple(win), absent=ab, **kwargs)


def unit_intervals(res):
    """``as_intervals`` of a result of ``unit``: the unit for ``line_products.from_results(intervals=...)``."""
    return as_intervals(res["top_depth"], res["base_depth"])


# ---- across lines: the survey graph -----------------------------------------------------------------------------------

MAX_SWEEPS = 65536
MAX_REFINE = 65536
MAX_CANDIDATES = 65536
SURVEY_OUTPUT = "survey.horizons.npz"


def graph_steps(x, y, surface, eu, ev, slope=0.05, min_distance=1.0):
    """(g, d, dist) float64 [E] of the edges ``eu[e]`` < ``ev[e]`` between soundings at ``x``, ``y`` (m) on the ``surface`` elevation
    (m): dist the horizontal distance, g[e] = 1 / (slope max(dist_e, min_distance)), d[e] = surface[ev[e]] - surface[eu[e]]: the
    convention of ``steps``, applied to an edge of the survey graph."""
    from . import sections
    x, y, s = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, surface))
    if not (x.size == y.size == s.size):
        raise ValueError("horizons.graph_steps: x, y and surface must have one entry per sounding")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(s))):
        raise ValueError("horizons.graph_steps: x, y and surface must be finite")
    slope, min_distance = float(slope), float(min_distance)
    if not (np.isfinite(slope) and slope > 0.0):
        raise ValueError("horizons.graph_steps: slope must be positive")
    if not (np.isfinite(min_distance) and min_distance > 0.0):
        raise ValueError("horizons.graph_steps: min_distance must be positive")
    eu, ev, _ = sections._check_edges(eu, ev, x.size, "horizons.graph_steps")
    dist = np.hypot(x[ev] - x[eu], y[ev] - y[eu])
    return 1.0 / (slope * np.maximum(dist, min_distance)), s[ev] - s[eu], dist


def _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what):
    """The checks the graph functions share, on shapes and host values alone (``score`` numpy or torch, any device); returns eu, ev
    (numpy int64 [E]), g, d (numpy float64 [E]), dz and switch."""
    from . import sections
    if getattr(score, "ndim", 0) != 2 or not 1 <= score.shape[1] <= MAX_STATES:
        raise ValueError("%s: score must be [N, S] with 1 <= S <= %d (choose a window with between=)" % (what, MAX_STATES))
    N = score.shape[0]
    if absent_score is not None and tuple(absent_score.shape) != (N,):
        raise ValueError("%s: absent_score must hold one entry per sounding" % what)
    eu, ev, _ = sections._check_edges(eu, ev, N, what)
    g, d = np.asarray(_args.host(g), dtype=np.float64).reshape(-1), np.asarray(_args.host(d), dtype=np.float64).reshape(-1)
    if g.size != eu.size or d.size != eu.size:
        raise ValueError("%s: g and d must hold one entry per edge (%d)" % (what, eu.size))
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(d))):
        raise ValueError("%s: g and d must be finite" % what)
    dz, switch = float(dz), float(switch)
    if not (np.isfinite(dz) and dz > 0.0):
        raise ValueError("%s: dz must be positive" % what)
    if not (np.isfinite(switch) and switch >= 0.0):
        raise ValueError("%s: switch must be >= 0" % what)
    return eu, ev, g, d, dz, switch


def _check_sweeps(sweeps, damping, what):
    from . import sections
    return _args.check_int(sweeps, 1, MAX_SWEEPS, "%s: sweeps" % what), sections._check_damping(damping, what)


def _theta_reference(score, absent_score, what):
    """The node terms as numpy float64 [N, SA], the absent state's last; they must be finite, as in ``track_reference``."""
    score = np.asarray(score, dtype=np.float64)
    theta = score if absent_score is None else np.concatenate([score, np.asarray(absent_score, dtype=np.float64).reshape(-1, 1)], axis=1)
    if not np.all(np.isfinite(theta)):
        raise ValueError("%s: the scores must be finite" % what)
    return theta


def _check_states(state, N, SA, most, what, name):
    """``state`` (host or device) as numpy int32 [R, N] with every entry in 0 .. SA - 1; also whether it came as one row [N]."""
    x = _args.host(state)
    single = x.ndim == 1
    x = x[None, :] if single else x
    if x.ndim != 2 or x.shape[1] != N or x.dtype.kind not in "iu" or not 1 <= x.shape[0] <= most:
        raise ValueError("%s: %s must hold one integer per sounding, [N] or [R, N] with N = %d and 1 <= R <= %d" % (what, name, N, most))
    if np.any(x < 0) or np.any(x >= SA):
        raise ValueError("%s: every entry of %s must lie in 0 .. %d (the states; %d with the absent state)" % (what, name, SA - 1, SA))
    return np.ascontiguousarray(x, dtype=np.int32), single


def _edge_tables(g, d, dz, S):
    """T_e[k + S - 1] = g[e] * |d[e] - k * dz|, k = -(S - 1) .. S - 1: the operations of ``track_reference``, in its order."""
    kf = np.arange(-(S - 1), S).astype(g.dtype)
    return [g[e] * np.abs(d[e] - kf * dz) for e in range(g.size)]


def _slots(table, S, i, mirror):
    """The table's entries for source cell i and every destination cell ascending: u -> v (``mirror`` False) reads slot
    b + S - 1 - i for b ascending, v -> u slot i - a + S - 1 for a ascending."""
    return table[i:i + S][::-1] if mirror else table[S - 1 - i:2 * S - 1 - i]


def _cost_to(T, switch, S, SA, dd, x):
    """The pair costs [SA] of the states of the sounding directed edge ``dd`` ends in, its source at state ``x``."""
    c = np.empty(SA, dtype=T.dtype)
    if x < S:
        c[:S] = _slots(T, S, x, bool(dd & 1))
        c[S:] = switch
    else:
        c[:S] = switch
        c[S:] = 0.0
    return c


def propagate_reference(eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=32, damping=0.0, dtype=np.float64):
    """The rule of ``propagate`` in numpy, evaluated in ``dtype`` (fp64: what the device is held to; np.longdouble: the yardstick of the
    rule's own rounding): synchronous sum-product message passing with the structure of ``sections.propagate_reference`` on the graph
    of N soundings with the undirected edges ``eu[e]`` < ``ev[e]`` (sorted by (eu, ev), no duplicates), ``g``, ``d`` [E]
    (``graph_steps``), ``score`` [N, S] and optionally ``absent_score`` [N] (SA = S + 1 states, the absent one last).

    w = exp(score); K_e = exp(-T_e) with T_e[k] = g[e] * |d[e] - k * dz|, k = b - a for cell a under eu[e] and cell b under ev[e];
    ks = exp(-switch).  Directed edge 2 e is eu -> ev, 2 e + 1 is ev -> eu and reads the same table mirrored.  A message has SA entries
    and starts at 1 / SA.  One sweep computes every message from the last sweep's.  For a -> b: h = w_a times the messages into a from
    its neighbours c != b, ascending c; for a cell j u[j] = sum_i h[i] K over the source cells i ascending, u = u + h[i] * K[..], then
    + h[S] * ks; for the absent state u[S] = the sequential sum of h[i] * ks over the cells, then + h[S]; tot = the sequential sum of u,
    j ascending; mu' = u / tot; with ``damping`` = lam != 0 mu' = (1 - lam) mu' + lam mu_old.  ``residual[t]`` is the largest
    |mu' - mu_old| of sweep t (NaN if a message is; 0.0 without edges).  belief_s = w_s times all incoming messages, divided by its
    sequential sum; ``state[s]`` is its first maximum.  A zero tot gives NaN.

    Exact on a forest once the sweeps reach its diameter (the residual is 0.0 from then on); on loops a belief, not a marginal.
    Returns ``belief`` [N, SA] (``dtype``), ``state`` int32 [N] and ``residual`` [sweeps]."""
    from . import sections
    what = "horizons.propagate_reference"
    ft = np.dtype(dtype).type
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, np.asarray(score), None if absent_score is None else np.asarray(absent_score), what)
    sweeps, damping = _check_sweeps(sweeps, damping, what)
    theta = _theta_reference(score, absent_score, what).astype(ft)
    N, SA = theta.shape
    S, E, has_absent = np.asarray(score).shape[1], eu.size, absent_score is not None
    g, d, dz, switch, lam = g.astype(ft), d.astype(ft), ft(dz), ft(switch), ft(damping)
    with np.errstate(under="ignore"):
        w, ks = np.exp(theta), np.exp(-switch)
        K = [np.exp(-T) for T in _edge_tables(g, d, dz, S)]
    inc, src = sections._neighbour_lists(eu, ev, N)
    dst = np.empty(2 * E, dtype=np.int64)
    dst[0::2], dst[1::2] = ev, eu
    msg = [np.full(SA, ft(1) / ft(SA), dtype=ft) for _ in range(2 * E)]
    residual = np.zeros(sweeps, dtype=ft)
    seq = lambda v: np.cumsum(v)[-1]                                          # noqa: E731  (sequential, ascending)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        for t in range(sweeps):
            new, r = [], ft(0)
            for dd in range(2 * E):
                a, b = int(src[dd]), int(dst[dd])
                h = w[a].copy()
                for q in inc[a]:                                             # ascending neighbour
                    if src[q] != b:
                        h = h * msg[q]
                Kd, u = K[dd // 2], np.zeros(SA, dtype=ft)
                for i in range(S):                                           # source cells ascending
                    u[:S] = u[:S] + h[i] * _slots(Kd, S, i, bool(dd & 1))
                if has_absent:
                    u[:S] = u[:S] + h[S] * ks
                    u[S] = seq(h[:S] * ks) + h[S]
                m = u / seq(u)
                if damping != 0.0:
                    m = (ft(1) - lam) * m + lam * msg[dd]
                r = sections._nan_max(r, np.abs(m - msg[dd]).max())
                new.append(m)
            msg = new
            residual[t] = r
        belief, state = np.zeros((N, SA), dtype=ft), np.zeros(N, dtype=np.int32)
        for s in range(N):
            h = w[s].copy()
            for q in inc[s]:
                h = h * msg[q]
            belief[s] = h / seq(h)
            state[s] = first_max(belief[s])
    return dict(belief=belief, state=state, residual=residual)


def _path_terms(eu, ev, g, d, dz, switch, score, absent_score, what):
    """The checked arguments of the max-sum rules and their terms: theta [N, SA] and the tables T_e, in fp64."""
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, np.asarray(score), None if absent_score is None else np.asarray(absent_score), what)
    theta = _theta_reference(score, absent_score, what)
    S = np.asarray(score).shape[1]
    return eu, ev, g, d, dz, switch, theta, S, _edge_tables(g, d, dz, S)


def _refine_rule(X, theta, T, switch, S, eu, ev, sweeps):
    """Coordinate ascent of one horizon ``X`` int32 [N], in place, with the move rule of ``sections.refine_reference``; returns the
    moves of every sweep, int32 [sweeps]."""
    from . import sections
    N, SA = theta.shape
    inc, src = sections._neighbour_lists(eu, ev, N)
    colour, n_colours = sections.sounding_colours(eu, ev, N)
    moves = np.zeros(sweeps, dtype=np.int32)
    for t in range(sweeps):
        for col in range(n_colours):
            for s in np.flatnonzero(colour == col):                           # (they share no edge: together is one after the other)
                v = theta[s].copy()
                for dd in inc[s]:                                             # ascending neighbour
                    v = v - _cost_to(T[dd >> 1], switch, S, SA, int(dd), int(X[src[dd]]))
                i, top = sections._first_above(v)
                if top > v[X[s]]:
                    X[s] = i
                    moves[t] += 1
        if moves[t] == 0:
            break
    return moves


def graph_log_score(state, eu, ev, g, d, dz, switch, score, absent_score=None):
    """The exact log score of the horizons ``state`` int [N] or [R, N] (S: absent) on the graph: the node terms score[s, x_s]
    (absent_score[s] for the absent state) summed over the soundings ascending, minus the pair costs summed over the edges ascending;
    both sums sequential in fp64 on the host, so the rule and the device give the same bits.  ``score`` (and ``absent_score``) numpy
    or torch on any device: only the [R, N] chosen node terms leave it.  Returns float64 numpy [R], or a number for one horizon."""
    what = "horizons.graph_log_score"
    if not torch.is_tensor(score):
        score, absent_score = np.asarray(score, dtype=np.float64), None if absent_score is None else np.asarray(_args.host(absent_score), dtype=np.float64)
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what)
    N, S = score.shape
    x, single = _check_states(state, N, S + (absent_score is not None), MAX_CANDIDATES + 1, what, "state")
    x = x.astype(np.int64)
    if torch.is_tensor(score):
        theta = score if absent_score is None else torch.cat([score, torch.as_tensor(absent_score).to(score.device, score.dtype).reshape(-1, 1)], dim=1)
        xt = torch.as_tensor(x).to(score.device)
        node = theta.to(torch.float64)[torch.arange(N, device=score.device)[None, :], xt].cpu().numpy()
    else:
        theta = np.asarray(score, dtype=np.float64)
        if absent_score is not None:
            theta = np.concatenate([theta, np.asarray(absent_score, dtype=np.float64).reshape(-1, 1)], axis=1)
        node = theta[np.arange(N)[None, :], x]
    xu, xv = x[:, eu], x[:, ev]
    cost = np.where((xu < S) & (xv < S), g[None, :] * np.abs(d[None, :] - (xv - xu).astype(np.float64) * dz),
                    np.where((xu >= S) & (xv >= S), 0.0, switch))
    total = lambda v: np.cumsum(v, axis=1)[:, -1] if v.shape[1] else np.zeros(v.shape[0])      # noqa: E731  (sequential, ascending)
    out = total(node) - total(cost)
    return out[0] if single else out


def refine_reference(state, eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=16):
    """The rule of ``refine`` in numpy: coordinate ascent on ``graph_log_score`` of the horizons ``state`` int [N] or [R, N].
    ``sections.sounding_colours`` colours the soundings; a sweep visits the colours in ascending order.  For sounding s,
    v[i] = score[s, i] minus the pair cost to the state of every neighbour, ascending neighbour; s moves to the first maximum of v
    (from -inf on strict >) only if v there is strictly greater than v[x_s].  A horizon stops after a sweep without a move.
    Returns ``state`` int32 (the shape given), ``refine_moves`` int32 [R, sweeps] ([sweeps] for one) and ``log_score``."""
    what = "horizons.refine_reference"
    eu, ev, g, d, dz, switch, theta, S, T = _path_terms(eu, ev, g, d, dz, switch, score, absent_score, what)
    sweeps = _args.check_int(sweeps, 0, MAX_REFINE, "%s: sweeps" % what)
    X, single = _check_states(state, theta.shape[0], theta.shape[1], MAX_CANDIDATES + 1, what, "state")
    X = X.copy()
    moves = np.stack([_refine_rule(X[r], theta, T, switch, S, eu, ev, sweeps) for r in range(X.shape[0])])
    ls = graph_log_score(X, eu, ev, g, d, dz, switch, score, absent_score)
    return dict(state=X[0] if single else X, refine_moves=moves[0] if single else moves, log_score=ls[0] if single else ls)


def graph_path_reference(eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=32, damping=0.0, refine=16, candidates=None):
    """The rule of ``graph_path`` in numpy (fp64: what the device is held to, bit for bit): the most probable horizon of the graph of
    ``propagate_reference`` -- the same arguments -- by synchronous max-sum message passing, a decode by conditioning and coordinate
    ascent, with the structure of ``sections.graph_path_reference``.  Everything is in the log domain; there is no exp.

    A message has SA entries and starts at 0.0.  For a -> b: h = score_a plus the messages into a from its neighbours c != b,
    ascending c; for a cell j u[j] = the maximum of h[i] - T over the source cells i ascending, from -inf and replaced on strict >,
    the candidate h[S] - switch last; for the absent state u[S] takes h[i] - switch for i ascending, then h[S]; nu' = u minus its first
    maximum; damping and ``residual`` as in ``propagate_reference``.  ``max_marginal`` [N, SA] = score_s plus all incoming messages,
    minus its maximum.  Decode: ``sections.decode_levels``; x_s = the first maximum of score_s[i] minus, per neighbour q ascending, the
    pair cost at x_q if level(q) < level(s), else plus nu[q -> s][i].  The decode and every row of ``candidates`` (int [C, N], states
    in 0 .. SA - 1) are refined by ``refine`` sweeps of ``refine_reference``; the first maximum of ``graph_log_score`` is kept.

    Returns ``state`` int32 [N] (S: absent), ``log_score``, ``max_marginal`` [N, SA], ``residual`` [sweeps], ``decoded_state``,
    ``candidate_state`` int32 [C + 1, N] (refined; row 0 from the decode), ``candidate_log_score`` [C + 1], ``chosen`` and
    ``refine_moves`` int32 [C + 1, refine]."""
    from . import sections
    what = "horizons.graph_path_reference"
    eu, ev, g, d, dz, switch, theta, S, T = _path_terms(eu, ev, g, d, dz, switch, score, absent_score, what)
    sweeps, damping = _check_sweeps(sweeps, damping, what)
    refine = _args.check_int(refine, 0, MAX_REFINE, "%s: refine" % what)
    N, SA = theta.shape
    E, has_absent = eu.size, SA > S
    given = None if candidates is None else _check_states(candidates, N, SA, MAX_CANDIDATES, what, "candidates")[0]
    inc, src = sections._neighbour_lists(eu, ev, N)
    dst = np.empty(2 * E, dtype=np.int64)
    dst[0::2], dst[1::2] = ev, eu
    msg = [np.zeros(SA) for _ in range(2 * E)]
    residual = np.zeros(sweeps)
    with np.errstate(invalid="ignore"):
        for t in range(sweeps):
            new, r = [], 0.0
            for dd in range(2 * E):
                a, b = int(src[dd]), int(dst[dd])
                h = theta[a].copy()
                for q in inc[a]:                                             # ascending neighbour
                    if src[q] != b:
                        h = h + msg[q]
                Td, u = T[dd // 2], np.full(SA, -np.inf)
                for i in range(S):                                           # source cells ascending, strict >
                    cand = h[i] - _slots(Td, S, i, bool(dd & 1))
                    u[:S] = np.where(cand > u[:S], cand, u[:S])
                if has_absent:
                    via = h[S] - switch
                    u[:S] = np.where(via > u[:S], via, u[:S])
                    top = sections._first_above(h[:S] - switch)[1]
                    u[S] = h[S] if h[S] > top else top
                m = u - sections._first_above(u)[1]
                if damping != 0.0:
                    m = (1.0 - damping) * m + damping * msg[dd]
                r = sections._nan_max(r, np.abs(m - msg[dd]).max())
                new.append(m)
            msg = new
            residual[t] = r
        max_marginal = np.empty((N, SA))
        for s in range(N):
            b = theta[s].copy()
            for q in inc[s]:
                b = b + msg[q]
            max_marginal[s] = b - sections._first_above(b)[1]
        level, level_ptr, level_node = sections.decode_levels(eu, ev, N)
        decoded = np.zeros(N, dtype=np.int32)
        for l in range(level_ptr.size - 1):
            picks = []
            for s in level_node[level_ptr[l]:level_ptr[l + 1]]:
                v = theta[s].copy()
                for dd in inc[s]:
                    q = src[dd]
                    v = v - _cost_to(T[dd >> 1], switch, S, SA, int(dd), int(decoded[q])) if level[q] < level[s] else v + msg[dd]
                picks.append(sections._first_above(v)[0])
            decoded[level_node[level_ptr[l]:level_ptr[l + 1]]] = picks
        X = decoded[None, :].copy() if given is None else np.concatenate([decoded[None, :], given])
        moves = np.stack([_refine_rule(X[r], theta, T, switch, S, eu, ev, refine) for r in range(X.shape[0])])
    ls = graph_log_score(X, eu, ev, g, d, dz, switch, score, absent_score)
    chosen = sections._first_above(ls)[0]
    return dict(state=X[chosen].copy(), log_score=ls[chosen], max_marginal=max_marginal, residual=residual, decoded_state=decoded, candidate_state=X,
                candidate_log_score=ls, chosen=chosen, refine_moves=moves)


def _device_graph(eu, ev, g, d, score, absent_score, module_what, entry):
    """The refusals of the device entries that come after the values (dtype, then the device last) and the tensors they share: theta
    [N, SA] (the absent state's score last), eu, ev, g, d and the CSR of incoming edges."""
    from . import sections
    if score.dtype != torch.float64 or (absent_score is not None and absent_score.dtype != torch.float64):
        raise TypeError("horizons.%s: score and absent_score are float64" % module_what)
    _args.on_device((score,) + (() if absent_score is None else (absent_score,)), "horizons", module_what, entry)
    dev = score.device
    theta = score.contiguous() if absent_score is None else torch.cat([score, absent_score.to(dev).reshape(-1, 1)], dim=1).contiguous()
    in_ptr, in_edge = sections.incoming(eu, ev, score.shape[0])
    t_eu, t_ev = (torch.as_tensor(a.astype(np.int32)).to(dev) for a in (eu, ev))
    return theta, t_eu, t_ev, torch.as_tensor(g).to(dev), torch.as_tensor(d).to(dev), torch.as_tensor(in_ptr).to(dev), torch.as_tensor(in_edge).to(dev)


def _are_tensors(score, absent_score, module_what, entry):
    _args.are_tensors((score,) + (() if absent_score is None else (absent_score,)), "horizons", module_what, entry)


def propagate(eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=32, damping=0.0):
    """Beliefs of the graph of ``propagate_reference`` on the device (gbp_horizon_graph_propagate: csrc/gbp_horizon_graph.h):
    ``score`` f64 [N, S] and ``absent_score`` f64 [N] or None on the device, S <= 2048; ``eu`` < ``ev`` [E] (sorted by (eu, ev), no
    duplicates), ``g``, ``d`` [E] (host or device; ``graph_steps``), ``dz`` > 0, ``switch`` >= 0, ``sweeps`` >= 1 synchronous sweeps
    with ``damping`` in [0, 1).  Returns on the device ``belief`` f64 [N, SA] (the absent state last), ``state`` int32 [N] (the first
    maximum of the belief; S: absent) and ``residual`` f64 [sweeps].  The two message buffers take 2 * 2 E * SA doubles.  There is no
    host fallback."""
    entry, what = "gbp_horizon_graph_propagate", "horizons.propagate"
    _are_tensors(score, absent_score, "propagate", entry)
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what)
    sweeps, damping = _check_sweeps(sweeps, damping, what)
    theta, t_eu, t_ev, t_g, t_d, t_ptr, t_edge = _device_graph(eu, ev, g, d, score, absent_score, "propagate", entry)
    dev, (N, SA), E = theta.device, theta.shape, eu.size
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(belief=torch.empty((N, SA), **f64), state=torch.empty(N, dtype=torch.int32, device=dev), residual=torch.zeros(sweeps, **f64))
    if N == 0:
        return out
    w, mu, resid = torch.empty((N, SA), **f64), torch.empty((2, 2 * E, SA), **f64), torch.empty((sweeps, 2 * E), **f64)
    _lib.call(entry, dev, N, E, score.shape[1], int(absent_score is not None), dz, switch, t_eu, t_ev, theta, t_g, t_d, t_ptr, t_edge, sweeps, damping,
              w, mu, resid, out["belief"], out["state"], out["residual"])
    return out


def _refine_on_device(X, graph, S, has_absent, dz, switch, eu, ev, sweeps):
    """gbp_horizon_graph_refine on the horizons ``X`` int32 [C, N] (device, contiguous), in place; returns the moves int32 [C, sweeps]."""
    from . import sections
    theta, t_eu, t_ev, t_g, t_d, t_ptr, t_edge = graph
    C, N = X.shape
    moves = torch.zeros((C, sweeps), dtype=torch.int32, device=X.device)
    if N == 0 or sweeps == 0:
        return moves
    colour_ptr, colour_node = sections._colour_lists(eu, ev, N)
    _lib.call("gbp_horizon_graph_refine", X.device, N, eu.size, S, has_absent, dz, switch, C, t_eu, t_ev, theta, t_g, t_d, t_ptr, t_edge,
              colour_ptr.size - 1, np.ctypeslib.as_ctypes(colour_ptr), torch.as_tensor(colour_node).to(X.device), sweeps, X, moves)
    return moves


def refine(state, eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=16):
    """Coordinate ascent on the exact log score on the device (gbp_horizon_graph_refine: csrc/gbp_horizon_graph.h k_hgraph_condition;
    ``refine_reference`` states the rule): the horizons ``state`` int [N] or [R, N] (host or device; S: absent) on the graph of
    ``propagate`` move sounding by sounding to their best state given their neighbours until a sweep moves nothing or ``sweeps``
    sweeps are done.  Returns on the device ``state`` int32 (the shape given) and ``refine_moves`` int32 [R, sweeps] ([sweeps] for
    one), and ``log_score`` (``graph_log_score``: float64 numpy [R], a number for one).  There is no host fallback."""
    entry, what = "gbp_horizon_graph_refine", "horizons.refine"
    _are_tensors(score, absent_score, "refine", entry)
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what)
    sweeps = _args.check_int(sweeps, 0, MAX_REFINE, "%s: sweeps" % what)
    S, has_absent = score.shape[1], int(absent_score is not None)
    X, single = _check_states(state, score.shape[0], S + has_absent, MAX_CANDIDATES + 1, what, "state")
    graph = _device_graph(eu, ev, g, d, score, absent_score, "refine", entry)
    X = torch.as_tensor(X).to(score.device)
    moves = _refine_on_device(X, graph, S, has_absent, dz, switch, eu, ev, sweeps)
    ls = graph_log_score(X, eu, ev, g, d, dz, switch, score, absent_score)
    return dict(state=X[0] if single else X, refine_moves=moves[0] if single else moves, log_score=ls[0] if single else ls)


def graph_path(eu, ev, g, d, dz, switch, score, absent_score=None, sweeps=32, damping=0.0, refine=16, candidates=None):
    """The most probable horizon of the graph of ``propagate`` on the device (gbp_horizon_graph_path and gbp_horizon_graph_refine:
    csrc/gbp_horizon_graph.h; ``graph_path_reference`` states the rule, and the device has its bits): the arguments of ``propagate``,
    max-sum sweeps in place of sum-product ones.  The decode is refined by up to ``refine`` sweeps of coordinate ascent, and so is
    every row of ``candidates`` (int [C, N], host or device; None: none); the refined horizon of the highest ``graph_log_score`` is
    returned.  Exact on a forest once the sweeps reach its diameter; on loops an approximation, never below any candidate given.

    Returns on the device ``state`` int32 [N] (S: absent), ``max_marginal`` f64 [N, SA], ``residual`` f64 [sweeps], ``decoded_state``
    int32 [N], ``candidate_state`` int32 [C + 1, N], ``refine_moves`` int32 [C + 1, refine]; on the host ``log_score`` (a number),
    ``candidate_log_score`` float64 [C + 1] and ``chosen``, an integer."""
    from . import sections
    entry, what = "gbp_horizon_graph_path", "horizons.graph_path"
    _are_tensors(score, absent_score, "graph_path", entry)
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what)
    sweeps, damping = _check_sweeps(sweeps, damping, what)
    refine = _args.check_int(refine, 0, MAX_REFINE, "%s: refine" % what)
    N, S = score.shape
    has_absent = int(absent_score is not None)
    SA, E = S + has_absent, eu.size
    given = None if candidates is None else _check_states(candidates, N, SA, MAX_CANDIDATES, what, "candidates")[0]
    graph = _device_graph(eu, ev, g, d, score, absent_score, "graph_path", entry)
    theta, t_eu, t_ev, t_g, t_d, t_ptr, t_edge = graph
    dev = theta.device
    f64 = dict(dtype=torch.float64, device=dev)
    max_marginal, residual, decoded = torch.empty((N, SA), **f64), torch.zeros(sweeps, **f64), torch.zeros(N, dtype=torch.int32, device=dev)
    if N:
        level, level_ptr, level_node = sections.decode_levels(eu, ev, N)
        nu, resid = torch.empty((2, 2 * E, SA), **f64), torch.empty((sweeps, 2 * E), **f64)
        _lib.call(entry, dev, N, E, S, has_absent, dz, switch, t_eu, t_ev, theta, t_g, t_d, t_ptr, t_edge, sweeps, damping, level_ptr.size - 1,
                  np.ctypeslib.as_ctypes(level_ptr), torch.as_tensor(level_node).to(dev), torch.as_tensor(level).to(dev), nu, resid, max_marginal,
                  decoded, residual)
    X = decoded[None, :].clone() if given is None else torch.cat([decoded[None, :], torch.as_tensor(given).to(dev)]).contiguous()
    moves = _refine_on_device(X, graph, S, has_absent, dz, switch, eu, ev, refine)
    ls = graph_log_score(X, eu, ev, g, d, dz, switch, score, absent_score)
    chosen = sections._first_above(ls)[0]
    return dict(state=X[chosen].clone(), log_score=ls[chosen], max_marginal=max_marginal, residual=residual, decoded_state=decoded, candidate_state=X,
                candidate_log_score=ls, chosen=chosen, refine_moves=moves)


def _check_graph_draw(eu, ev, g, d, dz, switch, score, absent_score, ptr, n_draws, seed, sweeps, row_key, state, first_sweep, what):
    """The host checks ``graph_draw`` and its reference share (shapes, dtypes, values).  Returns eu, ev, g, d, dz, switch, ptr,
    step_edge, cross, R, seed, sweeps, first_sweep, the keys (int64 [N]) and the states to continue from (int32 [R, N] or None)."""
    from . import sections
    eu, ev, g, d, dz, switch = _check_graph(eu, ev, g, d, dz, switch, score, absent_score, what)
    N, SA = score.shape[0], score.shape[1] + (absent_score is not None)
    ptr, step_edge, cross = sections.check_lines(eu, ev, ptr, N, what)
    R = _args.check_int(n_draws, 1, MAX_DRAWS, "%s: n_draws" % what)
    seed = sections._check_seed(seed)
    sweeps = _args.check_int(sweeps, 0, sections.MAX_DRAW_SWEEPS, "%s: sweeps" % what)
    first_sweep = _args.check_int(first_sweep, 0, sweeps, "%s: first_sweep (at most sweeps)" % what)
    key = sections._check_row_key(row_key, N, what)
    if (state is None) != (first_sweep == 0):
        raise ValueError("%s: state holds the states to continue from: it goes with first_sweep > 0, and only with it" % what)
    if state is not None:
        state, single = _check_states(state, N, SA, MAX_DRAWS, what, "state")
        if single or state.shape[0] != R:
            raise ValueError("%s: state must hold one integer per realisation and sounding [%d, %d]" % (what, R, N))
    return eu, ev, g, d, dz, switch, ptr, step_edge, cross, R, seed, sweeps, first_sweep, key, state


def graph_draw_reference(eu, ev, g, d, dz, switch, score, absent_score, ptr, n_draws, seed=0, sweeps=8, row_key=None, state=None, first_sweep=0,
                         dtype=np.float64):
    """The rule of ``graph_draw`` in numpy, evaluated in ``dtype``: R joint realisations of the horizon on the whole graph of
    ``propagate_reference`` by Gibbs sampling blocked by flight line, with the structure of ``sections.graph_draw_reference``
    (DESIGN.md 3.34).  The graph as there; ``ptr`` [L + 1]: the sequences (lines) in the same numbering, contiguous, possibly empty.

    Edges (``sections.check_lines``): an edge with ev = eu + 1 inside one sequence is a step, every other edge must join two different
    sequences, a cross edge; anything else is refused.  Colours: ``sections.line_colours``; cross CSRs: ``sections.cross_incoming``,
    neighbours ascending.
    Sweep 0, the start: ``draw_reference`` with the step edges' (g, d), cross edges ignored.
    Sweep t = 1 .. T: colours ascending; for every sequence of the colour and every realisation the same filter and walk with w' in
    place of w.  For each cross edge e of s in CSR order w'_s[i] is w_s[i] times the pair factor at the neighbour's current state x_q:
    exp(-(g_e * |d_e - k * dz|)) between cells, k = x_q - i for s = eu[e] and k = i - x_q for s = ev[e] (the orientation of
    ``_edge_tables`` / ``_cost_to``); ks between a cell and absent; absent-absent applies no multiply; the multiplies left to right.
    The step along the line uses the step edge's (g, d).  States are replaced in place.  u = ``sections.philox_uniform(seed, rho,
    row_key[s], sweep=t)``.  ``first_sweep`` > 0 continues from ``state`` int32 [R, N] and runs the sweeps first_sweep .. T.
    A draw depends on the seed, the realisation, the row key and the sweep -- not on R, on how realisations are cut into blocks or
    on a launch shape.  T = 8 is a convention, as in DESIGN.md 3.29, not a measured mixing time.

    Returns ``draw_state`` int32 [R, N] (S: absent), ``filtered`` [R, N, SA] (the alpha of the last sweep in which each sounding was
    drawn) and ``margin`` [R, N], the minimum over the sweeps run (the start's is its sequence's)."""
    from . import sections
    what = "horizons.graph_draw_reference"
    ft = np.dtype(dtype).type
    score = np.asarray(score, dtype=np.float64)
    has_absent = absent_score is not None
    absent_score = np.asarray(absent_score, dtype=np.float64).reshape(-1) if has_absent else None
    eu, ev, g, d, dz, switch, ptr, step_edge, cross, R, seed, T, first, key, state = _check_graph_draw(
        eu, ev, g, d, dz, switch, score, absent_score, ptr, n_draws, seed, sweeps, row_key, state, first_sweep, what)
    theta = _theta_reference(score, absent_score, what).astype(ft)
    N, SA = theta.shape
    S = score.shape[1]
    X = np.zeros((R, N), dtype=np.int32) if state is None else state.copy()
    filtered, margin = np.zeros((R, N, SA), dtype=ft), np.full((R, N), np.inf, dtype=ft)
    if first == 0:                                                            # the start: the chains of the steps alone
        has = step_edge >= 0
        gc, dc = np.ones(N), np.zeros(N)
        gc[has], dc[has] = g[step_edge[has]], d[step_edge[has]]
        start = draw_reference(ptr, score, absent_score, gc, dc, dz, switch, R, seed=seed, row_key=key, dtype=dtype)
        X[:], filtered[:] = start["draw_state"], start["filtered"][None, :, :]
        for l in range(ptr.size - 1):
            margin[:, ptr[l]:ptr[l + 1]] = start["margin"][:, l:l + 1]
    if T < max(first, 1):
        return dict(draw_state=X, filtered=filtered, margin=margin)
    g, d, dz, switch = g.astype(ft), d.astype(ft), ft(dz), ft(switch)
    kf = np.arange(-(S - 1), S).astype(ft)
    rho, cells = np.arange(R, dtype=np.int64), np.arange(S, dtype=np.int64)
    cross_ptr, cross_edge = sections.cross_incoming(eu, ev, cross, N)
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        w, ks = np.exp(theta), np.exp(-switch)

        def conditioned(s):
            """w' [R, SA] under the current states."""
            v = np.repeat(w[s][None, :], R, axis=0)
            for dd in cross_edge[cross_ptr[s]:cross_ptr[s + 1]]:              # ascending neighbour
                e, from_v = int(dd) >> 1, bool(dd & 1)
                x = X[:, ev[e] if from_v else eu[e]].astype(np.int64)
                k = (x[:, None] - cells[None, :]) if from_v else (cells[None, :] - x[:, None])
                fac = np.ones((R, SA), dtype=ft)                              # (times 1: no multiply)
                fac[:, :S] = np.where((x < S)[:, None], np.exp(-(g[e] * np.abs(d[e] - k.astype(ft) * dz))), ks)
                if has_absent:
                    fac[:, S] = np.where(x < S, ks, ft(1))
                v = v * fac
            return v

        for t in range(max(first, 1), T + 1):
            for c in range(n_colours):
                for l in np.flatnonzero(colour == c):
                    r0, n_l = int(ptr[l]), int(ptr[l + 1] - ptr[l])
                    if n_l == 0:
                        continue
                    alpha, Ks = [None] * n_l, []
                    v = conditioned(r0)
                    alpha[0] = v / v.sum(axis=1)[:, None]
                    for n in range(n_l - 1):
                        se = step_edge[r0 + n]
                        K = np.exp(-(g[se] * np.abs(d[se] - kf * dz)))
                        Ks.append(K)
                        a = alpha[n]
                        u = np.zeros((R, SA), dtype=ft)
                        for i in range(S):                                   # c ascending
                            u[:, :S] = u[:, :S] + a[:, i, None] * K[None, S - 1 - i:2 * S - 1 - i]
                        if has_absent:
                            u[:, :S] = u[:, :S] + (a[:, S] * ks)[:, None]
                            u[:, S] = np.cumsum(a[:, :S] * ks, axis=1)[:, -1] + a[:, S]
                        u = np.ascontiguousarray(conditioned(r0 + n + 1) * u)
                        alpha[n + 1] = u / u.sum(axis=1)[:, None]
                    j, new = None, np.zeros((R, n_l), dtype=np.int32)
                    for n in range(n_l - 1, -1, -1):
                        a = alpha[n]
                        filtered[:, r0 + n] = a
                        if n == n_l - 1:
                            W = a
                        else:
                            Kx = np.append(Ks[n], ks)                        # the switch in slot 2 S - 1
                            jc = j < S
                            W = np.empty((R, SA), dtype=ft)
                            W[:, :S] = a[:, :S] * Kx[np.where(jc[:, None], j[:, None] - cells[None, :] + (S - 1), 2 * S - 1)]
                            if has_absent:
                                W[:, S] = np.where(jc, a[:, S] * ks, a[:, S])
                        cs = np.cumsum(np.ascontiguousarray(W), axis=1, dtype=ft)      # sequential, i ascending
                        thr = sections.philox_uniform(seed, rho, key[r0 + n], sweep=t).astype(ft) * cs[:, -1]
                        j = np.minimum((cs <= thr[:, None]).sum(axis=1), SA - 1)
                        margin[:, r0 + n] = np.fmin(margin[:, r0 + n], np.abs(cs - thr[:, None]).min(axis=1) / cs[:, -1])
                        new[:, n] = j
                    X[:, r0:r0 + n_l] = new
    return dict(draw_state=X, filtered=filtered, margin=margin)


def graph_draw(eu, ev, g, d, dz, switch, score, absent_score, ptr, n_draws, seed=0, sweeps=8, row_key=None, state=None, first_sweep=0, block=None,
               budget_bytes=4 << 30, trace=False, filtered=False):
    """R joint realisations of the horizon on the whole survey graph on the device by Gibbs sampling blocked by flight line
    (gbp_horizon_graph_draw: csrc/gbp_horizon_draw.h; ``graph_draw_reference`` states the rule and what its draws are).  ``score`` f64
    [N, S] and ``absent_score`` f64 [N] or None on the device; ``eu``, ``ev``, ``g``, ``d`` as ``propagate`` takes them; ``ptr``
    [L + 1] (host): the lines; ``n_draws`` = R in 1 .. 65536, ``seed`` a uint64, ``sweeps`` = T in 0 .. 65535 (8 is a convention, not
    a measured mixing time), ``row_key`` int64 [N] (None: the index; several horizons of one survey: sounding index + horizon index
    * N, so that two horizons of one sounding never share a uniform).  ``first_sweep`` > 0 continues from ``state`` int32 [R, N] (host
    or device).  Realisations are independent chains whose random numbers depend on (seed, realisation, key, sweep): they are
    processed in blocks of ``block`` (None: as many as keep the block's alpha, R_b N SA 8 bytes, under ``budget_bytes``), and the
    blocking changes no draw.

    Returns on the device ``draw_state`` int32 [R, N] (S: absent) and, with ``filtered``, ``filtered`` f64 [R, N, SA].  ``trace`` runs
    sweep by sweep and adds ``log_score_trace`` f64 [T - first_sweep + 1, R] (``graph_log_score`` after every sweep that was run, the
    start included) and ``change_share`` f64 [T - max(first_sweep, 1) + 1]: the share of (realisation, sounding) pairs whose state a
    conditioned sweep changed.  There is no host fallback."""
    from . import sections
    entry, what = "gbp_horizon_graph_draw", "horizons.graph_draw"
    _are_tensors(score, absent_score, "graph_draw", entry)
    eu, ev, g, d, dz, switch, ptr, step_edge, cross, R, seed, T, first, key, state = _check_graph_draw(
        eu, ev, g, d, dz, switch, score, absent_score, ptr, n_draws, seed, sweeps, row_key, state, first_sweep, what)
    _args.check_block(block, what)
    budget_bytes = _args.check_int(budget_bytes, 1, 2 ** 62, "%s: budget_bytes" % what)
    theta, t_eu, t_ev, t_g, t_d, _, _ = _device_graph(eu, ev, g, d, score, absent_score, "graph_draw", entry)
    dev, (N, SA), E, L = theta.device, theta.shape, eu.size, ptr.size - 1
    S, has_absent = score.shape[1], int(absent_score is not None)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    per = int(block) if block is not None else max(1, min(R, budget_bytes // max(1, N * SA * 8)))
    per = min(per, R)
    out = dict(draw_state=torch.zeros((R, N), **i32) if state is None else torch.as_tensor(state).to(dev).contiguous())
    alpha = torch.zeros((R if filtered else per, N, SA), **f64)
    if filtered:
        out["filtered"] = alpha
    run_first = max(first, 1)
    if trace:
        out.update(log_score_trace=torch.zeros((T - first + 1, R), **f64), change_share=torch.zeros(max(T - run_first + 1, 0), **f64))
    if N == 0:
        return out
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    order = np.argsort(colour, kind="stable")
    colour_ptr = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))])
    cross_ptr, cross_edge = sections.cross_incoming(eu, ev, cross, N)
    to = lambda a, t=np.int32: torch.as_tensor(np.ascontiguousarray(a, dtype=t)).to(dev)      # noqa: E731
    t_step, t_cptr, t_colptr, t_colline = (to(a) for a in (step_edge, cross_ptr, colour_ptr, order))
    t_cedge = to(np.concatenate([cross_edge, [-1]]))                           # (never empty: the entry refuses a NULL pointer)
    t_ptr, t_key = to(ptr, np.int64), None if row_key is None else to(key, np.int64)
    scale = torch.empty((per, N), **f64)
    X = out["draw_state"]
    for a, b in ([(t, t) for t in range(first, T + 1)] if trace else [(first, T)]):
        before = X.clone() if trace and a >= 1 else None
        for r0 in range(0, R, per):
            r1 = min(R, r0 + per)
            _lib.call(entry, dev, N, E, S, has_absent, dz, switch, t_eu, t_ev, theta, t_g, t_d, L, t_ptr, t_step, t_cptr, t_cedge, n_colours, t_colptr,
                      t_colline, t_key, seed, r1 - r0, r0, a, b, alpha[r0:r1] if filtered else alpha[:r1 - r0], scale, X[r0:r1])
            if filtered and b == 0:                                           # the start alone: its one alpha serves every realisation
                alpha[r0:r1] = alpha[r0].clone()[None]
        if trace:
            out["log_score_trace"][a - first] = torch.as_tensor(np.atleast_1d(graph_log_score(X, eu, ev, g, d, dz, switch, score, absent_score))).to(dev)
            if before is not None:
                out["change_share"][a - run_first] = (X != before).double().mean()
    return out


def message_bytes(n_edges, n_states):
    """The bytes of the two message buffers [2, 2 E, SA] of float64 a graph launch holds."""
    return 2 * 2 * int(n_edges) * int(n_states) * 8


def spatial(evidence, x, y, surface, depth_edges, *, max_distance, ptr=None, absent=None, between=None, slope=0.05, switch=4.6, floor=1e-6,
            sweeps=32, damping=0.0, path=True, percentiles=(5, 50, 95), message_budget_bytes=8 << 30, draws=0, seed=0, draw_sweeps=8,
            row_key=None):
    """One horizon over the whole survey: the arguments of ``track`` -- ``evidence`` [N, n_depth] on the device, ``x``, ``y``,
    ``surface`` [N] on the host, the lines as ``ptr`` [L + 1] -- on the survey graph of ``sections.neighbours(x, y, ptr,
    max_distance=...)`` (``max_distance`` is required, about 1.5 line spacings; its ``g`` is discarded for ``graph_steps``).  The
    beliefs come from ``propagate`` (``sweeps``, ``damping``) and, with ``path``, the picks from ``graph_path`` with the same sweeps,
    its candidates being the first maximum of every belief and the lines tracked alone.

    Returns every entry of ``track`` as [N] -- ``cell`` int32 (index on the full axis; -1: absent), ``depth``, ``elevation``,
    ``marginal`` [N, S] (the beliefs of the window's cells), ``absent_probability``, ``depth_percentile_<p>`` -- with the picks from the
    chosen path (``path`` False: from the beliefs' first maxima), and ``log_score``, the path's ``graph_log_score``; beside them
    ``belief_cell`` int32 [N] (the first maximum of every belief, alone), ``state_log_score`` (its ``graph_log_score``, to compare),
    ``residual`` [sweeps], ``line_cell`` int32 [N] (the pick of ``track``, every line alone: what to compare against), ``edge_u``,
    ``edge_v``, ``edge_length``; and with ``path`` ``path_margin`` f64 [N] (the gap between the two largest max-marginals; inf with one
    state), ``path_residual`` [sweeps], ``path_candidate_log_score`` [3] (the refined decode, belief maxima and line picks) and
    ``path_chosen``.  The two message buffers hold 2 * 2 E * SA doubles; beyond ``message_budget_bytes`` (8 GiB by default: a
    convention, not a property of the device) a ValueError asks for a narrower window ``between=``.

    ``draws`` = R > 0 adds R joint realisations of the surface on the graph (``graph_draw`` with ``seed``, ``draw_sweeps`` = T sweeps
    -- 8 is a convention, as in DESIGN.md 3.29, not a measured mixing time -- and ``row_key``; None: the sounding index; for several
    horizons of one survey sounding index + horizon index * N): ``draw_cell`` int32 [R, N] (full axis; -1: absent), ``draw_depth``,
    ``draw_elevation`` [R, N] (NaN: absent), ``draw_log_score`` [R] (``graph_log_score`` of every realisation), ``draw_share``
    [N, SA] (the share of the realisations in every state, the absent one last: to be read against ``marginal`` /
    ``absent_probability``) and ``draw_change_share`` [T] (the share of states every sweep changed).  With ``draws`` = 0 every other
    output keeps its bits and nothing else is launched."""
    from . import sections
    ptr, g_line, d_line, switch = _track_arguments(evidence, x, y, surface, absent, slope, switch, floor, ptr)
    draws, seed = _check_draws(draws, seed, "horizons.spatial")
    draw_sweeps = _args.check_int(draw_sweeps, 0, sections.MAX_DRAW_SWEEPS, "horizons.spatial: draw_sweeps")
    sweeps, damping = _check_sweeps(sweeps, damping, "horizons.spatial")
    percentiles = check_percentiles(percentiles)
    edges, dz = check_depth_edges(depth_edges)
    if evidence.shape[1] != edges.size - 1:
        raise ValueError("horizons.spatial: evidence has %d depth cells, depth_edges %d" % (evidence.shape[1], edges.size - 1))
    lo, hi = window(edges, between)
    S, N = hi - lo, evidence.shape[0]
    SA = S + (absent is not None)
    if S > MAX_STATES:
        raise ValueError("horizons.spatial: %d states, at most %d (choose a window with between=)" % (S, MAX_STATES))
    eu, ev, _, dist = sections.neighbours(x, y, ptr, None, max_distance=max_distance)
    g, d, _ = graph_steps(x, y, surface, eu, ev, slope)
    if message_bytes(eu.size, SA) > int(message_budget_bytes):
        raise ValueError("horizons.spatial: the messages of %d edges and %d states take %d bytes, more than message_budget_bytes = %d; choose a "
                         "narrower window with between=" % (eu.size, SA, message_bytes(eu.size, SA), int(message_budget_bytes)))
    if evidence.device.type != "cuda":
        raise _lib.NativeLibraryError("horizons.spatial runs on the device (gbp_horizon_graph_propagate); there is no host fallback")
    dev = evidence.device
    score, absent_score = evidence_scores(evidence[:, lo:hi], absent, floor)
    score = score.contiguous()
    alone = _launch(score, absent_score, ptr, g_line, d_line, dz, switch, False)["cell"]
    found = propagate(eu, ev, g, d, dz, switch, score, absent_score, sweeps=sweeps, damping=damping)
    args = (eu, ev, g, d, dz, switch, score, absent_score)
    extra = {}
    if path:
        best = graph_path(*args, sweeps=sweeps, damping=damping, candidates=torch.stack([found["state"], alone]))
        state, log_score = best["state"], best["log_score"]
        two = torch.topk(best["max_marginal"], min(2, SA), dim=1).values
        margin = two[:, 0] - two[:, 1] if SA > 1 else torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
        extra = dict(path_margin=margin, path_residual=best["residual"], path_candidate_log_score=torch.as_tensor(best["candidate_log_score"]).to(dev),
                     path_chosen=torch.tensor(best["chosen"], dtype=torch.int32, device=dev))
    else:
        state, log_score = found["state"], graph_log_score(found["state"], *args)
    f64 = lambda v: torch.tensor(float(v), dtype=torch.float64, device=dev)    # noqa: E731
    raw = dict(cell=state, log_score=f64(log_score), marginal=found["belief"])
    if draws:
        drawn = graph_draw(*args, ptr, draws, seed=seed, sweeps=draw_sweeps, row_key=row_key, trace=True)
        X = drawn["draw_state"]
        count = torch.zeros((N, SA), dtype=torch.float64, device=dev).scatter_add_(1, X.long().T.contiguous(),
                                                                                   torch.ones((N, draws), dtype=torch.float64, device=dev))
        raw.update(draw_state=X, draw_log_score=drawn["log_score_trace"][-1])
        extra.update(draw_share=count / draws, draw_change_share=drawn["change_share"])
    out = _finish(raw, S, lo, edges, surface, percentiles)
    full_axis = lambda c: torch.where(c >= S, torch.full_like(c, -1), c + lo)  # noqa: E731
    out.update(belief_cell=full_axis(found["state"]), state_log_score=f64(graph_log_score(found["state"], *args)), residual=found["residual"],
               line_cell=full_axis(alone), edge_u=eu.astype(np.int32), edge_v=ev.astype(np.int32), edge_length=dist, **extra)
    return out


def spatial_from_products(paths, between, max_distance, slope=0.05, switch=4.6, floor=1e-6, sweeps=32, damping=0.0, path=True,
                          percentiles=(5, 50, 95), absent=False, device=None, message_budget_bytes=8 << 30, draws=0, seed=0, draw_sweeps=8):
    """``spatial`` for results containers (or saved line products with x, y and the surface beside them: what ``from_products`` reads):
    all ``paths`` given form ONE graph, every container a line, and one horizon is sought per window of ``between`` = [(d0, d1), ...].
    The containers must share their ``interface_depth_edges``.  The windows run one after the other (each has its own state count
    and its own graph launch).  Returns the entries of ``spatial`` stacked [H, N] (``log_score``, ``state_log_score``, ``path_chosen``
    [H]; ``residual``, ``path_residual``, ``path_candidate_log_score`` [H, ..]), ``marginal_<h>`` [N, S_h], ``between`` [H, 2], the
    graph's ``edge_u``, ``edge_v``, ``edge_length`` once, and ``ptr`` [L + 1], the containers' ranges of soundings.  ``draws`` = R > 0
    adds the draws of ``spatial`` -- ``draw_cell``, ``draw_depth``, ``draw_elevation`` [H, R, N], ``draw_log_score`` [H, R],
    ``draw_change_share`` [H, T] and ``draw_share_<h>`` [N, SA_h] -- with the row key sounding index + h * N for window h."""
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike, dict)) else list(paths)
    if not paths:
        raise ValueError("horizons.spatial_from_products: at least one container is needed")
    wins = [tuple(float(v) for v in w) for w in np.asarray(between, dtype=np.float64).reshape(-1, 2)]
    if not wins:
        raise ValueError("horizons.spatial_from_products: at least one window (d0, d1) is needed")
    read = [_read(p, None) for p in paths]
    for prob, edges, cx, cy, cs in read:
        if cx is None or cy is None or cs is None:
            raise ValueError("horizons.spatial_from_products: every container must hold x, y and the surface elevation")
        if edges.shape != read[0][1].shape or np.any(edges != read[0][1]):
            raise ValueError("horizons.spatial_from_products: the containers must share their interface_depth_edges")
        if prob.ndim != 2 or prob.shape[1] != edges.size - 1:
            raise ValueError("horizons.spatial_from_products: interface_probability %r does not match its %d depth cells" % (prob.shape, edges.size - 1))
    edges = read[0][1]
    prob = np.nan_to_num(np.concatenate([r[0] for r in read]), nan=0.0)
    x, y, surface = (np.concatenate([np.asarray(r[i], dtype=np.float64).reshape(-1) for r in read]) for i in (2, 3, 4))
    ptr = np.concatenate([[0], np.cumsum([r[0].shape[0] for r in read])]).astype(np.int64)
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    e = torch.as_tensor(prob).to(dev) if dev.type == "cuda" else torch.as_tensor(prob)
    parts = []
    for w in wins:
        lo, hi = window(edges, w)
        ab = (e.sum(1) - e[:, lo:hi].sum(1)).clamp(min=0.0) if absent else None
        parts.append(spatial(e, x, y, surface, edges, max_distance=max_distance, ptr=ptr, absent=ab, between=w, slope=slope, switch=switch, floor=floor,
                             sweeps=sweeps, damping=damping, path=path, percentiles=percentiles, message_budget_bytes=message_budget_bytes,
                             draws=draws, seed=seed, draw_sweeps=draw_sweeps,
                             row_key=np.arange(x.size, dtype=np.int64) + len(parts) * x.size if draws else None))
    out = {}
    for k in parts[0]:
        if k in ("marginal", "draw_share"):
            for h, p in enumerate(parts):
                out["%s_%d" % (k, h)] = p[k]
        elif k in ("edge_u", "edge_v", "edge_length"):
            out[k] = parts[0][k]
        else:
            out[k] = torch.stack([p[k] for p in parts])
    out["between"], out["ptr"] = np.asarray(wins, dtype=np.float64).reshape(-1, 2), ptr
    return out


def output_path(container):
    """``<line>.horizons.npz`` next to the container."""
    from .line_products import output_path as products_path
    return products_path(container)[:-len(".products.npz")] + OUTPUT_SUFFIX


def parser():
    ap = argparse.ArgumentParser(prog="python -m geobipy_amd.horizons",
                                 description="Track horizons along the lines of GeoBIPy results containers: per depth window the most "
                                             "probable path through the interface probability under a prior on the apparent dip, and its "
                                             "smoothed marginals, written to <line>.horizons.npz.")
    ap.add_argument("paths", nargs="+", help="results containers (<line>.h5, <line>.results.npz) or directories holding them")
    ap.add_argument("--between", type=float, nargs=2, action="append", metavar=("D0", "D1"), required=True,
                    help="a depth window (m below the surface) in which one horizon is sought; repeat for more horizons")
    ap.add_argument("--slope", type=float, default=0.05, help="scale of the apparent dip between neighbours, m per m (default 0.05)")
    ap.add_argument("--switch", type=float, default=4.6, help="price in nats of entering or leaving the absent state (default 4.6)")
    ap.add_argument("--absent", action="store_true", help="add the absent state, weighted by the interface probability outside the window")
    ap.add_argument("--no-marginals", action="store_true", help="only the picks: skip the forward-backward pass")
    ap.add_argument("--device", default=None, help="torch device of the kernels (default cuda:0)")
    ap.add_argument("--spatial", type=float, default=None, metavar="MAX_DISTANCE",
                    help="couple the lines: all containers given form one survey graph whose lines are joined across up to this distance (m; "
                         "about 1.5 line spacings), and survey.horizons.npz is written beside the first container")
    ap.add_argument("--sweeps", type=int, default=32, help="with --spatial: synchronous sweeps of message passing (default 32)")
    ap.add_argument("--damping", type=float, default=0.0, help="with --spatial: damping of the messages in [0, 1) (default 0)")
    ap.add_argument("--no-path", action="store_true", help="with --spatial: the picks are the beliefs' first maxima, not the max-sum path")
    ap.add_argument("--draws", type=int, default=0, metavar="R",
                    help="also draw R joint realisations of every horizon (draw_cell, draw_depth, draw_elevation, draw_log_score): every line "
                         "alone, or with --spatial on the survey graph")
    ap.add_argument("--seed", type=int, default=0, help="with --draws: the seed of the realisations (default 0)")
    ap.add_argument("--draw-sweeps", type=int, default=None, metavar="T",
                    help="with --spatial and --draws: sweeps of the line-blocked Gibbs sampler after the line-alone start (default 8: a "
                         "convention, not a measured mixing time)")
    ap.add_argument("--unit", action="store_true",
                    help="track the top and the base of ONE unit jointly in the one --between window, the base never above the top, and write "
                         "<line>.unit.npz instead")
    ap.add_argument("--min-thickness", type=float, default=None, metavar="M", help="with --unit: the least thickness (m; default one cell)")
    ap.add_argument("--coarsen", type=int, default=None, metavar="C", help="with --unit: sum groups of C cells before scoring (default 1)")
    ap.add_argument("--top-between", type=float, nargs=2, default=None, metavar=("A", "B"),
                    help="with --unit: the top's evidence counts only in this depth range")
    ap.add_argument("--base-between", type=float, nargs=2, default=None, metavar=("A", "B"),
                    help="with --unit: the base's evidence counts only in this depth range")
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.slope <= 0.0:
        ap.error("--slope must be positive")
    if a.switch < 0.0:
        ap.error("--switch must be >= 0")
    for d0, d1 in a.between:
        if not d0 < d1:
            ap.error("--between D0 D1 needs D0 < D1")
    if a.spatial is None and (a.sweeps != 32 or a.damping != 0.0 or a.no_path):
        ap.error("--sweeps, --damping and --no-path need --spatial MAX_DISTANCE")
    if a.spatial is not None and not (np.isfinite(a.spatial) and a.spatial > 0.0):
        ap.error("--spatial MAX_DISTANCE must be positive")
    if not 1 <= a.sweeps <= MAX_SWEEPS:
        ap.error("--sweeps must lie in 1 .. %d" % MAX_SWEEPS)
    if not 0.0 <= a.damping < 1.0:
        ap.error("--damping must lie in [0, 1)")
    if not 0 <= a.draws <= MAX_DRAWS:
        ap.error("--draws must lie in 0 .. %d" % MAX_DRAWS)
    if not 0 <= a.seed < 2 ** 64:
        ap.error("--seed must lie in 0 .. 2^64 - 1")
    if a.seed != 0 and a.draws == 0:
        ap.error("--seed needs --draws R")
    if a.draw_sweeps is not None and (a.spatial is None or a.draws == 0):
        ap.error("--draw-sweeps needs --spatial MAX_DISTANCE and --draws R (along a line alone a draw is exact: there are no sweeps)")
    if a.draw_sweeps is not None and not 0 <= a.draw_sweeps <= 65535:
        ap.error("--draw-sweeps must lie in 0 .. 65535")
    if not a.unit and (a.min_thickness is not None or a.coarsen is not None or a.top_between is not None or a.base_between is not None):
        ap.error("--min-thickness, --coarsen, --top-between and --base-between need --unit")
    if a.unit:
        if len(a.between) != 1:
            ap.error("--unit needs exactly one --between D0 D1: the window the top and the base share")
        if a.spatial is not None:
            ap.error("--unit tracks every line alone: pairs on the survey graph are not supported, drop --spatial")
        if a.draws:
            ap.error("--unit has no joint draws of pairs, drop --draws")
        if a.min_thickness is not None and not (np.isfinite(a.min_thickness) and a.min_thickness >= 0.0):
            ap.error("--min-thickness must be >= 0")
        if a.coarsen is not None and a.coarsen < 1:
            ap.error("--coarsen must be >= 1")
        for name, w in (("--top-between", a.top_between), ("--base-between", a.base_between)):
            if w is not None and not w[0] < w[1]:
                ap.error("%s A B needs A < B" % name)
    return a


def main(argv=None):
    from .line_products import containers
    a = parse_args(argv)
    if a.spatial is not None:
        found = [c for path in a.paths for c in containers(path)]
        r = spatial_from_products(found, a.between, a.spatial, slope=a.slope, switch=a.switch, sweeps=a.sweeps, damping=a.damping, path=not a.no_path,
                                  absent=a.absent, device=a.device, draws=a.draws, seed=a.seed, draw_sweeps=8 if a.draw_sweeps is None else a.draw_sweeps)
        written = [save(r, os.path.join(os.path.dirname(os.path.abspath(found[0])), SURVEY_OUTPUT))]
        print(written[0])
        return written
    written = []
    if a.unit:
        for path in a.paths:
            for c in containers(path):
                r = unit_from_products(c, a.between[0], absent=a.absent, device=a.device, slope=a.slope, switch=a.switch,
                                       marginals=not a.no_marginals, min_thickness=a.min_thickness, coarsen=1 if a.coarsen is None else a.coarsen,
                                       top_between=a.top_between, base_between=a.base_between)
                written.append(save(r, output_path(c)[:-len(OUTPUT_SUFFIX)] + UNIT_SUFFIX))
                print(written[-1])
        return written
    for path in a.paths:
        for c in containers(path):
            r = from_products(c, a.between, slope=a.slope, switch=a.switch, marginals=not a.no_marginals, absent=a.absent, device=a.device,
                              draws=a.draws, seed=a.seed)
            written.append(save(r, output_path(c)))
            print(written[-1])
    return written


if __name__ == "__main__":
    main()
