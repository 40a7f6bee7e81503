"""Local mixture fits of the hit maps and global classes (csrc/gbp_hitmap.h k_hitmap_mixture): what the reference's
mixture workflow does with one ``lmfit`` optimisation per column (Inference2D.fit_estimated_pdf / Inference3D.fit_mixture_to_pdf ->
Histogram.fit_mixture_to_pdf_2d -> Mixture.fit_to_curve, then Inference3D.cluster_fits_gmm and compute_probability).  The reference's
least-squares fit of Pearson-VII curves has an optimiser path that cannot be reproduced, so the rule is stated here on the host
(``mixture_reference``) and the kernel is held to it: the EM iteration of a 1-D Gaussian mixture on binned data, K = 1 .. Kmax components
each fitted from a quantile start ("stages"), and the reference's stopping rule (``select``) choosing the stage per column.  The local
means of a whole survey are then clustered into global classes (``global_classes``) in the form ``hitmap.class_probability`` takes.

    python -m geobipy_amd.mixtures <directory or <line>.products.npz files> --classes N [--bins 512] [--out global_classes.npz]

reads the ``mixture_mean`` of the lines' products (``python -m geobipy_amd.line_products ... --mixtures``), writes ``global_classes.npz``
(means, scales, weights, the histogram and its edges) and prints the matching ``--class-means ... --class-scales ...`` arguments.
"""
import argparse
import glob
import math
import os
import sys

import numpy as np
import torch

MAX_COMPONENTS = 4
MAX_ITERATIONS = 10000
MAX_CLASSES = 16
TINY = 10.0 * 2.0 ** -52                       # keeps a component without responsibility defined


def centres(n_value, half_width):
    """The value cells' centres ((v + 0.5) / n_value) 2 half_width - half_width, k_hitmap_stats's expression."""
    hw = float(half_width)
    return ((np.arange(int(n_value), dtype=np.float64) + 0.5) / float(n_value)) * (2.0 * hw) - hw


def _e_step(x, w, mu, s2):
    """(d [K, nv, C], l [K, nv, C], L [nv, C]) of parameters [K, C] at the centres x [nv]; the sum over the components adds them in
    ascending j."""
    d = x[None, :, None] - mu[:, None, :]
    ell = (np.log(w) - 0.5 * np.log(2.0 * np.pi * s2))[:, None, :] - d * d / (2.0 * s2)[:, None, :]
    top = ell.max(axis=0)
    return d, ell, top + np.log(np.add.reduce(np.exp(ell - top[None]), axis=0))


def _stage(c, x, N, K, n_iter, reg, dx):
    """Stage K of the rule for counts ``c`` [nv, C] (float64, exact integers) with totals ``N`` [C] (int64) over the centres ``x``
    [nv]: (weight, mean, variance) [K, C], loglik, ll_change [C], misfit [2, C].  Sums along the value axis add the rows in
    ascending v (a reduction over the leading axis).  Columns with N = 0 come out NaN."""
    nv, C = c.shape
    Nf = N.astype(np.float64)
    pos = c > 0
    with np.errstate(all="ignore"):
        m = np.add.reduce(c * x[:, None], axis=0) / Nf
        dm = x[:, None] - m[None, :]
        V = np.add.reduce(c * dm * dm, axis=0) / Nf
        if K == 1:
            w, mu, s2 = np.ones((1, C)), m[None, :].copy(), (V + reg)[None, :]
            ll_prev = None
        else:
            cum = np.cumsum(c.astype(np.int64), axis=0)
            idx = np.stack([(2 * K * cum < (2 * j + 1) * N[None, :]).sum(axis=0) for j in range(K)])      # int64: exact on both sides
            w = np.full((K, C), 1.0 / K)
            mu = x[np.minimum(idx, nv - 1)]
            s2 = np.tile((V / float(K * K) + reg)[None, :], (K, 1))
            ll_prev = np.zeros(C)
            for _ in range(int(n_iter)):
                d, ell, L = _e_step(x, w, mu, s2)
                r = np.where(pos[None], c[None] * np.exp(ell - L[None]), 0.0)
                ll_prev = np.add.reduce(np.where(pos, c * L, 0.0), axis=0) / Nf
                n = np.add.reduce(r, axis=1) + TINY
                A = np.add.reduce(r * d, axis=1)
                Q = np.add.reduce(r * d * d, axis=1)
                g = A / n
                mu = mu + g
                s2 = np.maximum(Q / n - g * g, 0.0) + reg
                nt = n[0].copy()
                for j in range(1, K):
                    nt = nt + n[j]
                w = n / nt[None, :]
        L = _e_step(x, w, mu, s2)[2]
        loglik = np.add.reduce(c * L, axis=0) / Nf
        p = c / Nf[None, :]
        e = np.abs(p - np.exp(L) * dx)
        misfit = np.stack([e.max(axis=0) / p.max(axis=0), np.sqrt(np.add.reduce(e * e, axis=0)) / np.sqrt(np.add.reduce(p * p, axis=0))])
        change = np.zeros(C) if ll_prev is None else loglik - ll_prev
    empty = N == 0
    nan = lambda a: np.where(empty, np.nan, a)                                    # noqa: E731
    return nan(w), nan(mu), nan(s2), nan(loglik), nan(change), nan(misfit)


def check_arguments(n_value, half_width, max_components, n_iter, reg):
    """(Kmax, n_iter, reg) checked, reg = dx^2 / 12 (a cell's own variance) when None."""
    hw = float(half_width)
    if not (math.isfinite(hw) and hw > 0.0):
        raise ValueError("mixture: half_width must be finite and positive, got %r" % (half_width,))
    K, n = int(max_components), int(n_iter)
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("mixture: max_components = %d, 1 .. %d are supported" % (K, MAX_COMPONENTS))
    if not 1 <= n <= MAX_ITERATIONS:
        raise ValueError("mixture: n_iter = %d outside 1 .. %d" % (n, MAX_ITERATIONS))
    dx = 2.0 * hw / int(n_value)
    reg = dx * dx / 12.0 if reg is None else float(reg)
    if not (math.isfinite(reg) and reg > 0.0):
        raise ValueError("mixture: reg must be finite and positive, got %r" % reg)
    return K, n, reg


def mixture_reference(maps, half_width, max_components=3, n_iter=50, reg=None):
    """The rule of ``hitmap.mixture`` on the host, in numpy, vectorised over the columns: ``maps`` [B, n_value, n_depth] integers.
    Returns the dict of ``hitmap.mixture`` as numpy arrays (``weight`` / ``mean`` / ``sd`` [B, Kmax (Kmax + 1) / 2, n_depth], ``loglik``
    / ``ll_change`` [B, Kmax, n_depth], ``misfit`` [B, Kmax, 2, n_depth]).

    Per column: counts c_v, N = sum c_v, centres x_v (``centres``, no prior shift), dx = 2 W / n_value.  Every stage K on its own:
    start w_j = 1 / K, mu_j = x at the first cell with 2 K cum_v >= (2 j + 1) N, s2_j = V / K^2 + reg (m, V: the column's mean and
    variance about it); ``n_iter`` EM iterations over the cells with c_v > 0 -- l_vj = ln w_j - ln(2 pi s2_j) / 2 - (x_v - mu_j)^2 /
    (2 s2_j), L_v = logsumexp_j, r_vj = c_v exp(l_vj - L_v); n_j = sum r + 10 * 2^-52, A = sum r d, Q = sum r d^2 about the old mean,
    mu_j += A / n_j, s2_j = max(Q / n_j - (A / n_j)^2, 0) + reg, w_j = n_j / sum n_j --; stage 1 is the closed form (1, m, V + reg),
    not iterated.  A closing pass over all cells: loglik = sum c_v L_v / N, ll_change = loglik minus the last E-step's (0 at stage 1),
    and with f_v = exp(L_v) dx, p_v = c_v / N: misfit = (max |p - f| / max p, ||p - f||_2 / ||p||_2).  N = 0: NaN."""
    h = np.asarray(maps)
    if h.ndim != 3 or h.dtype.kind not in "iu":
        raise TypeError("hit maps are integers [B, n_value, n_depth]")
    B, nv, nz = h.shape
    K, n_iter, reg = check_arguments(nv, half_width, max_components, n_iter, reg)
    x = centres(nv, half_width)
    dx = 2.0 * float(half_width) / nv
    ci = np.ascontiguousarray(h.astype(np.int64).transpose(1, 0, 2).reshape(nv, B * nz))
    N = ci.sum(axis=0)
    c = ci.astype(np.float64)
    S = K * (K + 1) // 2
    out = dict(weight=np.empty((B, S, nz)), mean=np.empty((B, S, nz)), sd=np.empty((B, S, nz)), loglik=np.empty((B, K, nz)),
               ll_change=np.empty((B, K, nz)), misfit=np.empty((B, K, 2, nz)))
    for k in range(1, K + 1):
        w, mu, s2, ll, ch, mf = _stage(c, x, N, k, n_iter, reg, dx)
        s0 = k * (k - 1) // 2
        out["weight"][:, s0:s0 + k] = w.reshape(k, B, nz).transpose(1, 0, 2)
        out["mean"][:, s0:s0 + k] = mu.reshape(k, B, nz).transpose(1, 0, 2)
        out["sd"][:, s0:s0 + k] = np.sqrt(s2).reshape(k, B, nz).transpose(1, 0, 2)
        out["loglik"][:, k - 1] = ll.reshape(B, nz)
        out["ll_change"][:, k - 1] = ch.reshape(B, nz)
        out["misfit"][:, k - 1] = mf.reshape(2, B, nz).transpose(1, 0, 2)
    return out


def _tensor(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def select(stages, epsilon=0.05, mu=0.1, log_mean_prior=None):
    """The stage of every column by the reference's stopping rule with its defaults: n = 1; while n < Kmax, stop unless both misfits
    of stage n exceed ``epsilon``; stage n + 1 is taken iff its misfit_2 is (strictly) smaller AND at least one of the two misfits
    changes by more than ``mu`` in absolute value, otherwise stop.  An empty column (NaN misfits) has n = 0.  Elementwise torch on the
    stages' device.  Returns ``n_components`` [B, n_depth] int32, ``weight`` / ``mean`` / ``sd`` [B, Kmax, n_depth] (the chosen
    stage's components sorted by mean ascending, stable; NaN beyond n_components; ``mean`` carries the prior shift log_mean_prior /
    ln 10 when ``log_mean_prior`` [B] is given), ``misfit`` [B, 2, n_depth], ``loglik`` and ``ll_change`` [B, n_depth] of that stage."""
    from .line_products import log10_shift
    st = {k: _tensor(v) for k, v in stages.items()}
    mf = st["misfit"]
    B, Kmax, _, nz = mf.shape
    dev = mf.device
    if st["weight"].shape[1] != Kmax * (Kmax + 1) // 2:
        raise ValueError("select: %d component slots do not belong to %d stages" % (st["weight"].shape[1], Kmax))
    active = ~(torch.isnan(mf[:, 0, 0]) | torch.isnan(mf[:, 0, 1]))
    n = active.to(torch.int64)
    eps, step = float(epsilon), float(mu)
    for k in range(1, Kmax):
        a, b = mf[:, k - 1], mf[:, k]
        go = active & (a[:, 0] > eps) & (a[:, 1] > eps) & (b[:, 1] < a[:, 1]) & (((b[:, 0] - a[:, 0]).abs() > step) | ((b[:, 1] - a[:, 1]).abs() > step))
        n = torch.where(go, torch.full_like(n, k + 1), n)
        active = go
    j = torch.arange(Kmax, device=dev)[None, :, None]
    valid = j < n[:, None, :]
    slot = torch.where(valid, (n * (n - 1) // 2)[:, None, :] + j, torch.zeros_like(j))               # [B, Kmax, nz]
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    mean = torch.where(valid, st["mean"].gather(1, slot), inf)
    mean, order = torch.sort(mean, dim=1, stable=True)
    sorted_valid = j < n[:, None, :]                                                                    # (the valid ones sort first)
    pick = lambda name: torch.where(sorted_valid, st[name].gather(1, slot).gather(1, order), nan)      # noqa: E731
    if log_mean_prior is not None:
        mean = mean + log10_shift(_tensor(log_mean_prior)).to(dev)[:, None, None]
    stage = (n - 1).clamp(min=0)
    some = n > 0
    per = lambda name: torch.where(some, st[name].gather(1, stage[:, None, :])[:, 0], nan)             # noqa: E731
    misfit = torch.where(some[:, None, :], mf.gather(1, stage[:, None, None, :].expand(B, 1, 2, nz))[:, 0], nan)
    return dict(n_components=n.to(torch.int32), weight=pick("weight"), mean=torch.where(sorted_valid, mean, nan), sd=pick("sd"),
                misfit=misfit, loglik=per("loglik"), ll_change=per("ll_change"))


def fit(maps, log_mean_prior, half_width, max_components=3, n_iter=50, reg=None, epsilon=0.05, mu=0.1):
    """``hitmap.mixture`` and ``select``: the local mixture fit of every column of ``maps`` [B, n_value, n_depth] on the maps' device
    (the dict of ``select``; means in log10 S/m with the prior shift)."""
    from . import hitmap
    return select(hitmap.mixture(maps, half_width, max_components, n_iter, reg), epsilon, mu, log_mean_prior=log_mean_prior)


def _means(fit_):
    for k in ("mixture_mean", "mean"):                               # (a line's products hold the posterior mean under 'mean')
        if k in fit_:
            return _tensor(fit_[k]).to(torch.float64)
    raise KeyError("a fit holds its local means under 'mean' (mixtures.fit) or 'mixture_mean' (line products)")


def global_classes(fits, n_classes, bins=512, n_iter=50):
    """Global classes from local fits -- the reference's ``cluster_fits_gmm`` in one dimension: every finite selected local mean of
    ``fits`` (one fit of ``fit`` / ``select``, or a list of them, one per line; the products of ``line_products.from_results(mixtures=
    ...)`` serve too), unweighted, goes into a histogram of ``bins`` cells over their range (on the fits' device, accumulated over the
    lines), and stage ``n_classes`` (1 .. 16) of the rule of ``mixture_reference`` is run on that one column.  Returns ``means``,
    ``scales`` (standard deviations), ``weights`` sorted by mean -- what ``hitmap.class_probability`` and
    ``line_products.check_classes`` take -- and ``histogram`` (int64 [bins]) with its ``edges``."""
    fits = [fits] if isinstance(fits, dict) else list(fits)
    K, bins = int(n_classes), int(bins)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError("global_classes: n_classes = %d, 1 .. %d are supported" % (K, MAX_CLASSES))
    if bins < 2:
        raise ValueError("global_classes: at least two bins")
    lo, hi = math.inf, -math.inf
    finite = []
    for f in fits:
        m = _means(f)
        m = m[torch.isfinite(m)]
        finite.append(m)
        if m.numel():
            lo, hi = min(lo, float(m.min())), max(hi, float(m.max()))
    if not lo <= hi:
        raise ValueError("global_classes: the fits hold no finite local mean")
    if not hi > lo:                                                   # (every mean the same: a unit range about it)
        lo, hi = lo - 0.5, hi + 0.5
    hist = np.zeros(bins, dtype=np.int64)
    for m in finite:
        if m.numel():
            hist += torch.histc(m, bins=bins, min=lo, max=hi).to(torch.int64).cpu().numpy()
    W, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    dx = 2.0 * W / bins
    w, mu, s2, _, _, _ = _stage(hist.astype(np.float64)[:, None], centres(bins, W), hist.sum(keepdims=True), K, int(n_iter), dx * dx / 12.0, dx)
    order = np.argsort(mu[:, 0], kind="stable")
    return dict(means=mu[order, 0] + mid, scales=np.sqrt(s2[order, 0]), weights=w[order, 0], histogram=hist,
                edges=np.linspace(lo, hi, bins + 1))


def products_files(paths):
    """The ``*.products.npz`` at ``paths``: the files themselves, or those of a directory, sorted."""
    found = []
    for p in paths:
        if os.path.isdir(p):
            found += sorted(glob.glob(os.path.join(p, "*.products.npz")))
        elif os.path.exists(p):
            found.append(p)
        else:
            raise FileNotFoundError(p)
    return found


def parser():
    ap = argparse.ArgumentParser(prog="python -m geobipy_amd.mixtures",
                                 description="Global classes from the local mixture fits of the lines' products (mixture_mean of "
                                             "<line>.products.npz, written by python -m geobipy_amd.line_products --mixtures).")
    ap.add_argument("paths", nargs="+", help="<line>.products.npz files or directories holding them")
    ap.add_argument("--classes", type=int, required=True, metavar="N", help="number of global classes, 1 to 16")
    ap.add_argument("--bins", type=int, default=512, help="cells of the histogram of local means (default 512)")
    ap.add_argument("--iterations", type=int, default=50, help="EM iterations (default 50)")
    ap.add_argument("--out", default=None, help="output file (default global_classes.npz in the first directory given, else beside the first file)")
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if not 1 <= a.classes <= MAX_CLASSES:
        ap.error("--classes must lie in 1 .. %d" % MAX_CLASSES)
    if a.bins < 2:
        ap.error("--bins must be at least 2")
    if not 1 <= a.iterations <= MAX_ITERATIONS:
        ap.error("--iterations must lie in 1 .. %d" % MAX_ITERATIONS)
    return a


def main(argv=None):
    a = parse_args(argv)
    files = products_files(a.paths)
    if not files:
        print("no *.products.npz under %s" % " ".join(a.paths), file=sys.stderr)
        return 1
    fits = []
    for f in files:
        with np.load(f) as z:
            if "mixture_mean" not in z:
                print("%s holds no mixture_mean (python -m geobipy_amd.line_products --mixtures writes it)" % f, file=sys.stderr)
                return 1
            fits.append(dict(mixture_mean=z["mixture_mean"]))
    try:
        g = global_classes(fits, a.classes, bins=a.bins, n_iter=a.iterations)
    except ValueError as e:
        print("mixtures: %s" % e, file=sys.stderr)
        return 1
    first = a.paths[0]
    dst = a.out or os.path.join(first if os.path.isdir(first) else os.path.dirname(os.path.abspath(first)), "global_classes.npz")
    np.savez_compressed(dst, **g)
    print("%d lines -> %s (%d local means)" % (len(files), dst, int(g["histogram"].sum())))
    print("--class-means %s --class-scales %s" % (" ".join("%.6g" % v for v in g["means"]), " ".join("%.6g" % v for v in g["scales"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
