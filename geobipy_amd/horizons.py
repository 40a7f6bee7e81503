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
is no host fallback for ``track`` itself.  Left out on purpose: coupling across lines, non-uniform depth cells, several horizons
tracked jointly with an ordering constraint, and learning ``slope`` (``log_partition`` is returned for whoever wants to scan it).
"""
import argparse

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


def _track_cells(evidence, absent, ptr, g, d, dz, switch, floor, marginals):
    """Scores of the (already windowed) evidence and the launch; the outputs are in cells of the window."""
    if evidence.shape[1] > MAX_STATES:
        raise ValueError("horizons.track: %d states, at most %d (choose a window with between=)" % (evidence.shape[1], MAX_STATES))
    if evidence.device.type != "cuda":
        raise _lib.NativeLibraryError("horizons.track runs on the device (gbp_horizon_track); there is no host fallback")
    score, absent_score = evidence_scores(evidence, absent, floor)
    return _launch(score, absent_score, ptr, g, d, dz, switch, marginals)


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
        out["log_partition"], out["scale"] = raw["log_partition"], raw["scale"]
    return out


def check_percentiles(percentiles):
    ps = tuple(float(p) for p in percentiles)
    if any(not 0.0 < p < 100.0 for p in ps):
        raise ValueError("horizons: percentiles must lie in (0, 100)")
    return ps


def track(evidence, x, y, surface, depth_edges, absent=None, between=None, slope=0.05, switch=4.6, floor=1e-6, marginals=True,
          percentiles=(5, 50, 95), ptr=None):
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
    ``scale`` [sum N] (s_n, the evidence of sounding n given those before it)."""
    ptr, g, d, switch = _track_arguments(evidence, x, y, surface, absent, slope, switch, floor, ptr)
    percentiles = check_percentiles(percentiles)
    edges, dz = check_depth_edges(depth_edges)
    if evidence.shape[1] != edges.size - 1:
        raise ValueError("horizons.track: evidence has %d depth cells, depth_edges %d" % (evidence.shape[1], edges.size - 1))
    lo, hi = window(edges, between)
    raw = _track_cells(evidence[:, lo:hi], absent, ptr, g, d, dz, switch, floor, marginals)
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
        else:
            out[k] = torch.stack([p[k] for p in parts])
    if between is not None:
        out["between"] = np.asarray(between, dtype=np.float64).reshape(-1, 2)
    return out


def _split(res, h, N):
    """Sequence ``h`` of a launch of sequences of N soundings each."""
    return {k: (v[h:h + 1] if k in ("log_score", "log_partition") else v[h * N:(h + 1) * N]) for k, v in res.items()}


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
                  marginals=True, percentiles=(5, 50, 95), absent=False, device=None):
    """One horizon per window of ``between`` = [(d0, d1), ...] through the ``interface_probability`` [N, n_depth] on
    ``interface_depth_edges`` of a results container (``<line>.h5``), of line products (a dict of ``line_products.from_results``) or
    of saved line products (``<line>.products.npz``); x, y and the surface elevation come from the ``container`` (with a container
    path as the first argument: that one) unless given.  ``absent`` = True adds the absent state with the weight of the probability
    mass outside the window.  The windows with equal cell counts run in one launch.  Returns the entries of ``track`` stacked
    [H, N] (``log_score``, ``log_partition`` [H]), ``marginal_<h>`` [N, S_h] and ``between`` [H, 2], on ``device`` (default cuda:0)."""
    prob, edges, cx, cy, cs = _read(path_or_products, container)
    x, y, surface = (cx if x is None else x), (cy if y is None else y), (cs if surface is None else surface)
    if x is None or y is None or surface is None:
        raise ValueError("horizons.from_products: x, y and surface are needed (give them, or a container that holds them)")
    wins = [tuple(float(v) for v in w) for w in np.asarray(between, dtype=np.float64).reshape(-1, 2)]
    if not wins:
        raise ValueError("horizons.from_products: at least one window (d0, d1) is needed")
    edges, dz = check_depth_edges(edges)
    percentiles = check_percentiles(percentiles)
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
        raw = _track_cells(ev, ab, ptr, g, d, dz, sw, floor, marginals)
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
    return a


def main(argv=None):
    from .line_products import containers
    a = parse_args(argv)
    written = []
    for path in a.paths:
        for c in containers(path):
            r = from_products(c, a.between, slope=a.slope, switch=a.switch, marginals=not a.no_marginals, absent=a.absent, device=a.device)
            written.append(save(r, output_path(c)))
            print(written[-1])
    return written


if __name__ == "__main__":
    main()
