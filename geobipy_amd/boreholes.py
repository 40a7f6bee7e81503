"""Borehole logs as evidence for sections: the log weight every kept model of a sounding gets from the logs that stand near it
(csrc/gbp_boreholes.h k_borehole_score through gbp_borehole_score).

``sections``, ``draw``, ``propagate`` and ``graph_draw`` take a ``score``: a log weight per kept model per sounding.  This module
produces one from the one piece of ground truth an airborne survey has.  A log is attached to ONE sounding per flight line, the
nearest; the chain and the survey graph carry it along and across the lines.

``Logs``             Nb boreholes: ``x``, ``y``, ``collar`` [Nb] (the elevation of depth 0; NaN where only depths are known), ``ptr``
                     [Nb + 1], and per interval ``top``, ``bottom`` (m below the collar), ``value`` (log10 S/m), ``sd`` (decades) and
                     ``cls``.  A MEASURED interval has a value, sd > 0 and cls = -1 (an induction log); a LITHOLOGY interval has cls
                     >= 0 and NaN for value and sd (a driller's log, read against ``classes``).
``load`` / ``save``  ``.npz`` with these arrays, or a text table ``name,x,y,collar,top,bottom,value,sd,class`` with one interval per
                     row (the rows of a borehole follow each other; an empty field or ``nan`` is NaN, an empty class is -1; a borehole
                     without intervals has no row, so only the ``.npz`` keeps it).
``attach``           which sounding every borehole speaks to (host, numpy): the nearest sounding with models of every sequence within
                     ``max_distance``, with the variance ``tau^2 d / length`` that the offset d adds -- the random walk of
                     ``sections.steps``, no new number -- and the ``shift`` between the collar and the sounding's ground.
``score_reference``  the rule in numpy, in any dtype.
``score``            the same on the device, one kernel: ``score`` f64 [S, n], ``part`` f64 [A, n], ``skipped`` int32 [A].
``log_predictive``   ln sum_m w_m exp(part[a, m]) per attachment: under the weights of a section that has NOT seen the log, how well the
                     section predicts it -- a blind test with a number per borehole.

The rule.  For kept model m < n_used[s] of sounding s with k layers, interfaces e and a_l = log10 sigma_l, for every attachment a of s
in order (borehole b, variance var, shift) and every interval of b in order:
  t' = max(top + shift, 0), b' = bottom + shift.  An interval with b' <= t' lies above the sounding's ground: it is skipped and counted
  in ``skipped[a]``.  h = b' - t'.  The segments [p, q] are the merge of [t', b'] with the model's layers: l starts at the number of
  interfaces <= t'; q = fmin(e_l, b') (e_l = +inf in the last layer); the layer advances where e_l == q; p = q; until p >= b'.
  MEASURED:   mean = (sum (q - p) a_l) / h;  term = -((mean - value)^2) / (2 (sd^2 + var)).
  LITHOLOGY of class c:  l_q(x) = ln pi_q - 0.5 ln v_q - (x - mu_q)^2 / (2 v_q) with v_q = s_q^2 + var (the walk broadens every class
              alike);  P_l = 1 / sum_q exp(l_q(a_l) - l_c(a_l)), q ascending;  Pbar = (sum (q - p) P_l) / h;
              term = ln(class_floor + (1 - class_floor) Pbar): with probability ``class_floor`` a log entry says nothing -- a smooth
              floor, no decision at a boundary.
  part[a, m] = the sum of the attachment's terms, score[s, m] = the sum of its parts in attachment order; 0.0 for a sounding without
  attachments, for m >= n_used[s] and for an absent model (row outside the slots, k <= 0).
Two conventions are chosen, not fitted.  Constants common to all models of a sounding are dropped (the Gaussian's -ln(sd sqrt(2 pi))
per interval): every weight of the sounding moves alike, so paths, marginals and draws do not see them and ``log_partition`` shifts by
them.  The interval mean is taken in log10 conductivity, the project's decades, not in conductivity -- an induction tool averages
something between the two, and the distance of ``families`` is in decades as well.  ``classes`` = (means, scales[, priors]) in log10
S/m, 1 to 16 classes as in ``line_products``; the priors (default 1 each) enter as ln pi and need not sum to 1: only their ratios count.
The interfaces of a model ascend (the sampler keeps them so): the kernel counts the interfaces <= t' by walking on from the interval
before.

Left out on purpose: deviated wells (a log is vertical under its collar), fitting ``tau`` or ``sd``, wiring into ``survey.infer``,
feeding logs back into the sampler's prior.  There is no host fallback: ``score`` refuses tensors that are not on the device."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._args import are_tensors, check_block, check_ensemble, host, on_device
from ._args import check_ptr as _check_ptr

MAX_MODELS = 1024
MAX_K = 64
MAX_CLASSES = 16
ENTRY = "gbp_borehole_score"
COLUMNS = ("name", "x", "y", "collar", "top", "bottom", "value", "sd", "class")
ATT_KEYS = ("att_ptr", "att_sounding", "att_bore", "att_var", "att_shift", "att_distance")


def _number(v, what, positive=True):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or (positive and not v > 0):
        raise ValueError("boreholes: %s must be a %s number" % (what, "positive finite" if positive else "finite"))
    return float(v)


# ---- logs ---------------------------------------------------------------------------------------------------------------------------

class Logs:
    """Nb boreholes and their I intervals (the module's docstring); every array is checked and every refusal names what is wrong."""

    def __init__(self, x, y, collar, ptr, top, bottom, value=None, sd=None, cls=None, name=None):
        f = lambda a: np.array(a, dtype=np.float64).reshape(-1)               # noqa: E731
        self.x, self.y, self.top, self.bottom = f(x), f(y), f(top), f(bottom)
        Nb, I = self.x.size, self.top.size
        self.collar = np.full(Nb, np.nan) if collar is None else f(collar)
        self.value = np.full(I, np.nan) if value is None else f(value)
        self.sd = np.full(I, np.nan) if sd is None else f(sd)
        c = np.full(I, -1) if cls is None else np.asarray(cls).reshape(-1)
        if c.dtype.kind not in "iu":
            raise ValueError("boreholes.Logs: cls must hold integers (-1: a measured interval)")
        self.cls = c.astype(np.int32)
        if self.y.size != Nb or self.collar.size != Nb:
            raise ValueError("boreholes.Logs: x, y and collar must hold one entry per borehole (%d)" % Nb)
        if not (np.all(np.isfinite(self.x)) and np.all(np.isfinite(self.y))):
            raise ValueError("boreholes.Logs: x and y must be finite")
        if np.any(np.isinf(self.collar)):
            raise ValueError("boreholes.Logs: collar must be finite, or NaN where only depths are known")
        p = np.asarray(ptr)
        if p.ndim != 1 or p.size != Nb + 1 or p.dtype.kind not in "iu":
            raise ValueError("boreholes.Logs: ptr must be a vector of Nb + 1 integers")
        p = p.astype(np.int64)
        if p[0] != 0 or p[-1] != I or np.any(np.diff(p) < 0):
            raise ValueError("boreholes.Logs: ptr must start at 0, end at the number of intervals (%d) and not decrease" % I)
        self.ptr = p
        if not (self.bottom.size == self.value.size == self.sd.size == self.cls.size == I):
            raise ValueError("boreholes.Logs: top, bottom, value, sd and cls must hold one entry per interval (%d)" % I)
        if not (np.all(np.isfinite(self.top)) and np.all(np.isfinite(self.bottom))):
            raise ValueError("boreholes.Logs: top and bottom must be finite")
        if np.any(self.top < 0.0) or np.any(self.bottom <= self.top):
            raise ValueError("boreholes.Logs: every interval needs 0 <= top < bottom (metres below the collar)")
        inner = np.ones(I, dtype=bool)
        inner[p[:-1][p[:-1] < I]] = False                                      # the first interval of a borehole has none before it
        if I > 1 and np.any(self.top[1:][inner[1:]] < self.bottom[:-1][inner[1:]]):
            raise ValueError("boreholes.Logs: the intervals of a borehole must ascend and must not overlap (gaps are allowed)")
        if np.any(self.cls < -1):
            raise ValueError("boreholes.Logs: cls must be -1 (measured) or a class >= 0")
        measured = self.cls < 0
        if np.any(~np.isfinite(self.value[measured])) or np.any(~(np.isfinite(self.sd[measured]) & (self.sd[measured] > 0.0))):
            raise ValueError("boreholes.Logs: a measured interval (cls = -1) needs a finite value and a finite sd > 0")
        if np.any(~np.isnan(self.value[~measured])) or np.any(~np.isnan(self.sd[~measured])):
            raise ValueError("boreholes.Logs: an interval is of exactly one kind: a lithology interval (cls >= 0) holds NaN for value and sd")
        if name is None:
            self.name = None
        else:
            self.name = [str(v) for v in np.asarray(name).reshape(-1)]
            if len(self.name) != Nb:
                raise ValueError("boreholes.Logs: name must hold one entry per borehole (%d)" % Nb)

    @property
    def n_boreholes(self):
        return self.x.size

    @property
    def n_intervals(self):
        return self.top.size

    def arrays(self):
        out = dict(x=self.x, y=self.y, collar=self.collar, ptr=self.ptr, top=self.top, bottom=self.bottom, value=self.value, sd=self.sd, cls=self.cls)
        if self.name is not None:
            out["name"] = np.array(self.name, dtype=str)
        return out


def _is_table(path):
    return not str(path).endswith(".npz")


def save(logs, path):
    """Write ``logs`` to ``path``: ``.npz`` with the arrays of ``Logs``, any other name the text table of the module's docstring
    (numbers with 17 significant digits: a round trip keeps every bit).  Returns the path."""
    if not isinstance(logs, Logs):
        raise ValueError("boreholes.save: logs must be a boreholes.Logs")
    path = os.fspath(path)
    if not _is_table(path):
        np.savez_compressed(path, **logs.arrays())
        return path
    if np.any(np.diff(logs.ptr) == 0):
        raise ValueError("boreholes.save: the text table has one row per interval and cannot hold a borehole without intervals; write .npz")
    names = logs.name if logs.name is not None else ["BH%d" % b for b in range(logs.n_boreholes)]
    if len(set(names)) != len(names) or any("," in v or "\n" in v or not v.strip() for v in names):
        raise ValueError("boreholes.save: the text table needs distinct, non-empty names without commas")
    num = lambda v: "" if np.isnan(v) else repr(float(v))                      # noqa: E731
    with open(path, "w") as f:
        f.write(",".join(COLUMNS) + "\n")
        for b in range(logs.n_boreholes):
            for i in range(int(logs.ptr[b]), int(logs.ptr[b + 1])):
                f.write(",".join([names[b], num(logs.x[b]), num(logs.y[b]), num(logs.collar[b]), num(logs.top[i]), num(logs.bottom[i]),
                                  num(logs.value[i]), num(logs.sd[i]), str(int(logs.cls[i]))]) + "\n")
    return path


def load(path):
    """``Logs`` from a file ``save`` wrote, or from a hand-made one of either format; ``path`` may be a ``Logs`` (returned as it is)."""
    if isinstance(path, Logs):
        return path
    path = os.fspath(path)
    if not _is_table(path):
        with np.load(path) as f:
            missing = [n for n in ("x", "y", "ptr", "top", "bottom") if n not in f.files]
            if missing:
                raise ValueError("boreholes.load: %s holds no %s" % (path, ", ".join(missing)))
            g = lambda n: f[n] if n in f.files else None                       # noqa: E731
            return Logs(f["x"], f["y"], g("collar"), f["ptr"], f["top"], f["bottom"], g("value"), g("sd"), g("cls"), g("name"))
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("#")]
    if not lines or tuple(c.strip().lower() for c in lines[0].split(",")) != COLUMNS:
        raise ValueError("boreholes.load: %s must start with the header %s" % (path, ",".join(COLUMNS)))
    names, x, y, collar, ptr, cols = [], [], [], [], [0], [[] for _ in range(5)]

    def num(text, row, col, blank=np.nan):
        text = text.strip()
        if not text:
            return blank
        try:
            return float(text)
        except ValueError:
            raise ValueError("boreholes.load: %s row %d: %s is not a number (%r)" % (path, row, col, text)) from None

    for r, line in enumerate(lines[1:], start=2):
        cell = line.split(",")
        if len(cell) != len(COLUMNS):
            raise ValueError("boreholes.load: %s row %d: %d fields, the table has %d" % (path, r, len(cell), len(COLUMNS)))
        nm = cell[0].strip()
        if not nm:
            raise ValueError("boreholes.load: %s row %d: the name is empty" % (path, r))
        head = [num(cell[1], r, "x"), num(cell[2], r, "y"), num(cell[3], r, "collar")]
        if not names or nm != names[-1]:
            if nm in names:
                raise ValueError("boreholes.load: %s row %d: the rows of borehole %s do not follow each other" % (path, r, nm))
            names.append(nm)
            x.append(head[0]), y.append(head[1]), collar.append(head[2])
            ptr.append(ptr[-1])
        elif not np.array_equal(np.array(head), np.array([x[-1], y[-1], collar[-1]]), equal_nan=True):
            raise ValueError("boreholes.load: %s row %d: borehole %s changes its x, y or collar" % (path, r, nm))
        c = num(cell[8], r, "class", blank=-1.0)
        if c != np.floor(c):
            raise ValueError("boreholes.load: %s row %d: class must be an integer (-1 or empty: a measured interval)" % (path, r))
        for dst, v in zip(cols, (num(cell[4], r, "top"), num(cell[5], r, "bottom"), num(cell[6], r, "value"), num(cell[7], r, "sd"), c)):
            dst.append(v)
        ptr[-1] += 1
    return Logs(x, y, collar, np.array(ptr, dtype=np.int64), cols[0], cols[1], cols[2], cols[3], np.array(cols[4], dtype=np.int64), names)


# ---- attachment ---------------------------------------------------------------------------------------------------------------------

def attach(x, y, logs, ptr=None, n_used=None, *, max_distance, surface=None, tau=0.1, length=100.0):
    """Which sounding every borehole of ``logs`` speaks to (host, numpy): of every sequence of ``ptr`` [L + 1] (None: one sequence) the
    NEAREST sounding among those with ``n_used`` > 0 (None: all), if it lies within ``max_distance`` in the horizontal; a tie goes to
    the lower index.  One sounding per line is the convention of ``sections.neighbours``: a log is not counted once per neighbour along
    a line -- the chain carries it.  ``max_distance`` is required and is not guessed.

    An attachment holds the sounding, the borehole, the distance d, ``var`` = tau^2 d / length (decades^2: the random walk of
    ``sections.steps``, ``tau`` decades per ``length`` metres; d = 0 gives 0) and ``shift`` = surface[s] - collar[b] with ``surface``
    [S] (the elevation of the ground under every sounding; a NaN collar is then refused), else 0: depths below the collar are depths
    below the sounding's ground.  Returns a dictionary sorted by sounding, then borehole, as a CSR: ``att_ptr`` int32 [S + 1],
    ``att_sounding`` / ``att_bore`` int32 [A], ``att_var`` / ``att_shift`` / ``att_distance`` f64 [A]."""
    if not isinstance(logs, Logs):
        raise ValueError("boreholes.attach: logs must be a boreholes.Logs (boreholes.load reads a file)")
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != y.size:
        raise ValueError("boreholes.attach: x and y must have one entry per sounding")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("boreholes.attach: x and y must be finite")
    S = x.size
    max_distance, tau, length = _number(max_distance, "max_distance"), _number(tau, "tau"), _number(length, "length")
    p = np.array([0, S] if S else [0], dtype=np.int64) if ptr is None else _check_ptr(ptr, S, "boreholes")
    nu = np.ones(S, dtype=np.int64) if n_used is None else host(n_used).reshape(-1)
    if nu.size != S or nu.dtype.kind not in "iu":
        raise ValueError("boreholes.attach: n_used must hold one integer per sounding")
    if surface is not None:
        surface = np.asarray(surface, dtype=np.float64).reshape(-1)
        if surface.size != S or not np.all(np.isfinite(surface)):
            raise ValueError("boreholes.attach: surface must hold one finite elevation per sounding")
        if np.any(np.isnan(logs.collar)):
            raise ValueError("boreholes.attach: surface is given, so every borehole needs a collar elevation (borehole %d has NaN)"
                             % int(np.flatnonzero(np.isnan(logs.collar))[0]))
    pairs = []
    for a, b in zip(p[:-1], p[1:]):
        members = a + np.flatnonzero(nu[a:b] > 0)
        if not members.size:
            continue
        D = np.hypot(logs.x[:, None] - x[members][None, :], logs.y[:, None] - y[members][None, :])       # [Nb, members]
        j = np.argmin(D, axis=1) if logs.n_boreholes else np.zeros(0, dtype=np.int64)   # the first minimum: the lowest index
        d = D[np.arange(logs.n_boreholes), j]
        for bore in np.flatnonzero(d <= max_distance):
            pairs.append((int(members[j[bore]]), int(bore), float(d[bore])))
    pairs.sort()
    s = np.array([q[0] for q in pairs], dtype=np.int32)
    bore = np.array([q[1] for q in pairs], dtype=np.int32)
    dist = np.array([q[2] for q in pairs], dtype=np.float64)
    att_ptr = np.zeros(S + 1, dtype=np.int32)
    np.cumsum(np.bincount(s, minlength=S), out=att_ptr[1:])
    shift = surface[s] - logs.collar[bore] if surface is not None else np.zeros(s.size)
    return dict(att_ptr=att_ptr, att_sounding=s, att_bore=bore, att_var=(tau * tau) * dist / length, att_shift=shift, att_distance=dist)


def check_attachment(att, S, Nb, what):
    """``att`` (what ``attach`` returns) against S soundings and Nb boreholes; returns its arrays in the entry's dtypes."""
    if not isinstance(att, dict) or any(k not in att for k in ATT_KEYS):
        raise ValueError("%s: att is what boreholes.attach returns (%s)" % (what, ", ".join(ATT_KEYS)))
    p = np.asarray(att["att_ptr"])
    if p.ndim != 1 or p.size != S + 1 or p.dtype.kind not in "iu":
        raise ValueError("%s: att_ptr must hold S + 1 = %d integers" % (what, S + 1))
    s, b = np.asarray(att["att_sounding"]).reshape(-1), np.asarray(att["att_bore"]).reshape(-1)
    var, shift = (np.asarray(att[k], dtype=np.float64).reshape(-1) for k in ("att_var", "att_shift"))
    A = s.size
    if b.size != A or var.size != A or shift.size != A or s.dtype.kind not in "iu" or b.dtype.kind not in "iu":
        raise ValueError("%s: att_sounding, att_bore, att_var and att_shift must hold one entry per attachment" % what)
    if p[0] != 0 or p[-1] != A or np.any(np.diff(p) < 0):
        raise ValueError("%s: att_ptr must start at 0, end at the number of attachments (%d) and not decrease" % (what, A))
    if not np.array_equal(s, np.repeat(np.arange(S), np.diff(p))):
        raise ValueError("%s: att_sounding must be the sounding of every attachment in the order of att_ptr" % what)
    if np.any(b < 0) or np.any(b >= Nb):
        raise ValueError("%s: att_bore must lie in 0 .. Nb - 1 = %d" % (what, Nb - 1))
    if not np.all(np.isfinite(var) & (var >= 0.0)) or not np.all(np.isfinite(shift)):
        raise ValueError("%s: att_var must be finite and >= 0, att_shift finite" % what)
    return p.astype(np.int32), s.astype(np.int32), b.astype(np.int32), var, shift


def check_classes(classes, logs, class_floor, what):
    """``classes`` = (means, scales[, priors]) or None as (means, scales, priors) float64 [C] (C = 0: none), and ``class_floor``."""
    if isinstance(class_floor, bool) or not isinstance(class_floor, (int, float, np.integer, np.floating)) or not 0.0 < class_floor < 1.0:
        raise ValueError("%s: class_floor must lie in (0, 1)" % what)
    top = int(logs.cls.max(initial=-1))
    if classes is None:
        if top >= 0:
            raise ValueError("%s: the logs hold lithology intervals (class %d); they need classes=(means, scales[, priors])" % (what, top))
        return np.zeros(0), np.zeros(0), np.zeros(0), float(class_floor)
    if not isinstance(classes, (tuple, list)) or len(classes) not in (2, 3):
        raise ValueError("%s: classes is (means, scales) or (means, scales, priors)" % what)
    from .line_products import check_classes as two
    mu, sd = two(classes[0], classes[1])
    pr = np.ones(mu.size) if len(classes) == 2 else np.asarray(classes[2], dtype=np.float64).reshape(-1)
    if pr.size != mu.size or not np.all(np.isfinite(pr) & (pr > 0.0)):
        raise ValueError("%s: classes: as many priors as means, finite and positive" % what)
    if top >= mu.size:
        raise ValueError("%s: the logs name class %d, classes holds %d" % (what, top, mu.size))
    return mu, sd, pr, float(class_floor)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------

def score_reference(k, edges, sigma, rows, n_used, att, logs, classes=None, class_floor=1e-6, dtype=np.float64, terms=False):
    """The rule of the module's docstring in numpy, evaluated in ``dtype`` (fp64: the device's arithmetic; np.longdouble: the yardstick
    the device is held to).  ``k`` [S, n_slots], ``edges`` / ``sigma`` [S, n_slots, K], ``rows`` [S, n], ``n_used`` [S], ``att`` of
    ``attach``, ``logs`` a ``Logs``.  Returns ``score`` [S, n], ``part`` [A, n] in ``dtype`` and ``skipped`` int32 [A]; with ``terms``
    also ``terms``: per attachment an array [intervals of its borehole, n] of the single terms (0.0 where skipped or absent), and
    ``peaks``, of the same shape: the largest |a_l| (measured) or P_l (lithology) among the interval's segments -- what a test needs
    to say how far a rounded interval end can move a term."""
    ft = np.dtype(dtype).type
    k, edges, sigma, rows = np.asarray(k), np.asarray(edges, dtype=np.float64), np.asarray(sigma, dtype=np.float64), np.asarray(rows)
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or edges.shape[:2] != k.shape or rows.ndim != 2 or rows.shape[0] != k.shape[0]:
        raise ValueError("boreholes.score_reference: k [S, n_slots], edges and sigma [S, n_slots, K], rows [S, n]")
    if not isinstance(logs, Logs):
        raise ValueError("boreholes.score_reference: logs must be a boreholes.Logs")
    S, ns = k.shape
    K, n = edges.shape[2], rows.shape[1]
    nu = host(n_used).reshape(-1)
    if nu.size != S or nu.dtype.kind not in "iu":
        raise ValueError("boreholes.score_reference: n_used must hold one integer per sounding")
    att_ptr, _, att_bore, att_var, att_shift = check_attachment(att, S, logs.n_boreholes, "boreholes.score_reference")
    mu, sc, pr, floor = check_classes(classes, logs, class_floor, "boreholes.score_reference")
    mu, sc, lnpi, floor = mu.astype(ft), sc.astype(ft), np.log(pr.astype(ft)), ft(floor)      # (ln of the priors in the rule's precision)
    A = att_bore.size
    score, part, skipped = np.zeros((S, n), dtype=ft), np.zeros((A, n), dtype=ft), np.zeros(A, dtype=np.int32)
    all_terms, all_peaks = [None] * A, [None] * A
    zero, one, two, half, inf = ft(0), ft(1), ft(2), ft(0.5), ft(np.inf)
    at = np.arange(n)
    for s in range(S):
        if att_ptr[s] == att_ptr[s + 1]:
            continue
        r = rows[s].astype(np.int64)
        inside = (at < min(max(int(nu[s]), 0), n)) & (r >= 0) & (r < ns)
        src = np.clip(r, 0, ns - 1)
        kk = np.where(inside, np.clip(k[s, src], 0, K), 0)
        active = kk > 0
        layer = np.arange(K)[None, :]
        E = np.where(layer < kk[:, None] - 1, edges[s, src], np.inf).astype(ft)                      # [n, K]: +inf from k - 1 on
        with np.errstate(divide="ignore", invalid="ignore"):
            V = np.where(layer < kk[:, None], np.log10(np.where(layer < kk[:, None], sigma[s, src], 1.0).astype(ft)), ft(np.nan))
        last = np.maximum(kk - 1, 0)
        for a in range(int(att_ptr[s]), int(att_ptr[s + 1])):
            b, var, shift = int(att_bore[a]), ft(att_var[a]), ft(att_shift[a])
            v = sc * sc + var
            cst, two_v = lnpi - half * np.log(v), two * v
            i0, i1 = int(logs.ptr[b]), int(logs.ptr[b + 1])
            acc_part = np.zeros(n, dtype=ft)
            mine, peaks = np.zeros((i1 - i0, n), dtype=ft), np.zeros((i1 - i0, n), dtype=ft)
            held = {}
            for i in range(i0, i1):
                tp, bp = max(ft(logs.top[i]) + shift, zero), ft(logs.bottom[i]) + shift
                if bp <= tp:
                    skipped[a] += 1
                    continue
                c = int(logs.cls[i])
                h = bp - tp
                if c < 0:
                    F = V
                else:
                    if c not in held:                                          # P of every layer of every model under class c
                        with np.errstate(over="ignore", invalid="ignore"):
                            dc = V - mu[c]
                            lc = cst[c] - (dc * dc) / two_v[c]
                            tot = np.zeros(V.shape, dtype=ft)
                            for q in range(mu.size):                           # q ascending
                                d = V - mu[q]
                                tot = tot + np.exp((cst[q] - (d * d) / two_v[q]) - lc)
                            held[c] = one / tot
                    F = held[c]
                li = np.minimum((E <= tp).sum(axis=1), last)
                p, acc, peak = np.full(n, tp, dtype=ft), np.zeros(n, dtype=ft), np.zeros(n, dtype=ft)
                for _ in range(K + 1):
                    live = active & (p < bp)
                    if not live.any():
                        break
                    ni = np.where(li < kk - 1, E[at, li], inf)
                    q = np.fmin(ni, bp)
                    with np.errstate(invalid="ignore"):
                        acc = np.where(live, acc + (q - p) * F[at, li], acc)
                        peak = np.where(live, np.fmax(peak, np.abs(F[at, li])), peak)
                    li = np.where(live & (ni == q), li + 1, li)
                    p = np.where(live, q, p)
                mean = acc / h
                if c < 0:
                    d = mean - ft(logs.value[i])
                    e = ft(logs.sd[i])
                    term = -(d * d) / (two * (e * e + var))
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        term = np.log(floor + (one - floor) * mean)
                term = np.where(active, term, zero)
                mine[i - i0] = term
                peaks[i - i0] = peak
                acc_part = acc_part + term
            part[a] = acc_part
            score[s] = score[s] + acc_part
            all_terms[a], all_peaks[a] = mine, peaks
    out = dict(score=score, part=part, skipped=skipped)
    if terms:
        out["terms"], out["peaks"] = all_terms, all_peaks
    return out


# ---- the device ---------------------------------------------------------------------------------------------------------------------

def score(ens, rows, n_used, att, logs, classes=None, class_floor=1e-6, block=None):
    """The rule on the device (gbp_borehole_score): ``ens`` an ensemble on the device, ``rows`` int32 [S, n] and ``n_used`` int32 [S] on
    the device (``families.used_rows``), ``att`` of ``attach``, ``logs`` a ``Logs``, ``classes`` = (means, scales[, priors]) for
    lithology intervals.  Returns on the device ``score`` f64 [S, n], ``part`` f64 [A, n] and ``skipped`` int32 [A].  ``block``:
    soundings per launch (None: one launch); the bits are the same."""
    are_tensors((ens.k, ens.edges, ens.sigma, rows, n_used), "boreholes", "score", ENTRY)
    k, edges, sigma, S, ns, K = check_ensemble(ens, batch="S", rows=rows, what="boreholes.score", max_rows=MAX_MODELS)
    if ns < 1 or not 1 <= K <= MAX_K:
        raise ValueError("ensemble: at least one slot and K in [1, %d]" % MAX_K)
    if tuple(n_used.shape) != (S,) or n_used.dtype != torch.int32:
        raise ValueError("boreholes.score: n_used is int32 [S]")
    if not isinstance(logs, Logs):
        raise ValueError("boreholes.score: logs must be a boreholes.Logs (boreholes.load reads a file)")
    att_ptr, _, att_bore, att_var, att_shift = check_attachment(att, S, logs.n_boreholes, "boreholes.score")
    mu, sc, pr, floor = check_classes(classes, logs, class_floor, "boreholes.score")
    lnpi = np.log(pr)
    check_block(block, "boreholes.score")
    on_device((k, edges, sigma, rows, n_used), "boreholes", "score", ENTRY)
    dev = k.device
    rows, n_used = rows.contiguous(), n_used.contiguous()
    n, A, Nb, I, C = rows.shape[1], att_bore.size, logs.n_boreholes, logs.n_intervals, mu.size
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    t_bore, t_var, t_shift = up(att_bore, np.int32), up(att_var, np.float64), up(att_shift, np.float64)
    t_bptr = up(logs.ptr, np.int32)
    t_top, t_bottom, t_value, t_sd, t_cls = (up(logs.top, np.float64), up(logs.bottom, np.float64), up(logs.value, np.float64),
                                             up(logs.sd, np.float64), up(logs.cls, np.int32))
    as_c = lambda a: (ctypes.c_double * max(C, 1))(*a)                   # noqa: E731
    c_mu, c_sc, c_ln = as_c(mu), as_c(sc), as_c(lnpi)
    out = dict(score=torch.empty((S, n), dtype=torch.float64, device=dev), part=torch.empty((A, n), dtype=torch.float64, device=dev),
               skipped=torch.empty(A, dtype=torch.int32, device=dev))
    step = S if block is None else int(block)
    for s0 in range(0, S, max(step, 1)):
        s1 = min(S, s0 + step)
        a0, a1 = int(att_ptr[s0]), int(att_ptr[s1])
        _lib.call(ENTRY, dev, s1 - s0, ns, K, k[s0:s1], edges[s0:s1], sigma[s0:s1], n, rows[s0:s1], n_used[s0:s1], a1 - a0,
                  up(att_ptr[s0:s1 + 1] - att_ptr[s0], np.int32), t_bore[a0:a1] if a1 > a0 else None, t_var[a0:a1] if a1 > a0 else None,
                  t_shift[a0:a1] if a1 > a0 else None, Nb, t_bptr, I, t_top if I else None, t_bottom if I else None, t_value if I else None,
                  t_sd if I else None, t_cls if I else None, C, c_mu, c_sc, c_ln, floor, out["score"][s0:s1],
                  out["part"][a0:a1] if a1 > a0 else None, out["skipped"][a0:a1] if a1 > a0 else None)
    return out


def log_predictive(part, weight, n_used, att):
    """ln sum_m w_m exp(part[a, m]) f64 [A] per attachment, m over the n_used models of the attachment's sounding: ``part`` f64 [A, n]
    of ``score``, ``weight`` f64 [S, n] (the smoothed marginals or beliefs of a section) and ``n_used`` [S] on the device, ``att`` of
    ``attach``.  A stable log-sum-exp in torch.  Under the weights of an UNCONDITIONED section this is the log predictive density of
    the log (up to the constants the rule drops): how well the section predicts a log it has not seen."""
    are_tensors((part, weight, n_used), "boreholes", "log_predictive", "torch")
    if part.ndim != 2 or weight.ndim != 2 or part.shape[1] != weight.shape[1] or n_used.shape != (weight.shape[0],):
        raise ValueError("boreholes.log_predictive: part [A, n], weight [S, n], n_used [S]")
    s = np.asarray(att["att_sounding"]).reshape(-1)
    if s.size != part.shape[0] or (s.size and (s.min() < 0 or s.max() >= weight.shape[0])):
        raise ValueError("boreholes.log_predictive: att_sounding must hold one sounding in 0 .. S - 1 per row of part")
    dev = part.device
    idx = torch.as_tensor(s.astype(np.int64)).to(dev)
    inside = torch.arange(part.shape[1], device=dev)[None, :] < n_used.to(dev)[idx][:, None].long()
    x = torch.log(weight.to(dev)[idx]) + part
    x = torch.where(inside, x, torch.full((), -float("inf"), dtype=part.dtype, device=dev))
    return torch.logsumexp(x, dim=1) if s.size else torch.zeros(0, dtype=part.dtype, device=dev)


# ---- the keyword of sections --------------------------------------------------------------------------------------------------------

OPTION_KEYS = ("logs", "max_distance", "surface", "classes", "class_floor")


def check_options(options, what):
    """``boreholes=`` of ``sections.sections`` / ``sections.spatial``: dict(logs=, max_distance=, surface=None, classes=None,
    class_floor=1e-6) with ``logs`` a ``Logs`` or a path; checked before any device work."""
    if not isinstance(options, dict) or "logs" not in options or "max_distance" not in options or not set(options) <= set(OPTION_KEYS):
        raise ValueError("%s: boreholes is a dictionary with logs and max_distance and optionally surface, classes and class_floor" % what)
    logs = load(options["logs"])
    floor = options.get("class_floor", 1e-6)
    check_classes(options.get("classes"), logs, floor, what + ": boreholes")
    return dict(logs=logs, max_distance=_number(options["max_distance"], "max_distance"), surface=options.get("surface"),
                classes=options.get("classes"), class_floor=floor)


def section_score(ens, rows, n_used, x, y, ptr, options, tau, length):
    """What ``sections`` and ``spatial`` do with the checked ``options``: attach and score.  Returns (score tensor, att, part, skipped)."""
    att = attach(x, y, options["logs"], ptr, host(n_used), max_distance=options["max_distance"], surface=options["surface"], tau=tau, length=length)
    res = score(ens, rows, n_used, att, options["logs"], classes=options["classes"], class_floor=options["class_floor"])
    return res["score"], att, res["part"], res["skipped"]


def section_outputs(att, bscore, part, skipped, weight, n_used):
    """The ``borehole_*`` entries of a section's result; ``weight`` None (no marginals): no ``borehole_log_predictive``."""
    dev = bscore.device
    out = dict(borehole_score=bscore, borehole_sounding=torch.as_tensor(att["att_sounding"]).to(dev), borehole_index=torch.as_tensor(att["att_bore"]).to(dev),
               borehole_distance=torch.as_tensor(att["att_distance"]).to(dev), borehole_skipped=skipped)
    if weight is not None:
        out["borehole_log_predictive"] = log_predictive(part, weight, n_used, att)
    return out
