"""Laterally coherent sections of sampled models along flight lines (csrc/gbp_ensemble_families.h
k_layered_cross_distance, csrc/gbp_section.h k_section_viterbi / k_section_marginals).

``families`` hands on one kept model per sounding; where a posterior has two families of comparable share that pick jumps between them
from one sounding to the next, and nothing per sounding can say which branch continues along the line.  Here one kept model per
sounding is chosen JOINTLY along a line: the states of a Markov chain under sounding s are its kept models (``families.used_rows``),
and the step s -> s + 1 from model i to model j costs g[s] D^2(i, j), D the RMS difference in decades of the two layered models over
the depth window (the distance of ``families.distance``, between the models of two different soundings).

``partners``        which sounding each sounding is paired with: the next of its sequence, -1 at a sequence's end and around soundings
                    without models.
``cross_distance``  D^2 (or D) f64 [S, n, n] between the models of every sounding and those of its partner, one kernel
                    (gbp_ensemble_cross_distance; ``cross_distance_reference`` states the rule through ``families.distance_reference``).
``steps``           g[s] = length / (2 tau^2 max(dx_s, min_distance)): the RMS difference between neighbouring models is taken as a
                    random walk of standard deviation ``tau`` decades per ``length`` metres, so that -g D^2 is its Gaussian log
                    density.  ``tau`` = 0.1 per 100 m and the 1 m floor are a documented convention, not fitted numbers.
``track``           the most probable path (Viterbi) and the smoothed marginals (forward-backward) of that chain (gbp_section_track;
                    ``track_reference`` states the rule in numpy: the device is held to it with ``==`` for the path and its score and to
                    the rule's own rounding for the marginals).
``sections``        all of the above for an ensemble, and the chosen models: a section made of models the sampler visited, as continuous
                    along the line as the posteriors allow, with the weight every sounding's models get from their neighbours.
``from_survey``     the same for a ``survey.SurveyResult`` (or its saved file) that carries the ensemble; sequences are the flight lines.
``draw``            joint draws of whole sections from the chain's posterior by forward filtering and backward sampling (DESIGN.md 3.26;
                    gbp_section_draw: csrc/gbp_section.h k_section_filter / k_section_draw; ``draw_reference`` states the rule and
                    ``philox_uniform`` its random numbers).  ``sections(..., draws=R, seed=N)`` adds them to its result, ``draw_models``
                    gathers their models (and rasters them), and ``exceedance_area`` is one product that needs them: the area of a
                    section above a conductivity threshold, a quantity of the line with a posterior only over joint realisations.
``lateral_products``  the laterally informed posterior of every sounding on a depth axis (gbp_ensemble_weighted through
                    ``ensembles.weighted``): the weighted mean, sd, percentiles and exceedance probabilities of log10 conductivity
                    per depth cell, the kept models weighted by the smoothed marginals ``weight``.  ``sections(..., products=dict(
                    depth_edges=...))`` adds them to its result: a section of medians with a credible band.

The rule of the chain.  A launch holds L sequences concatenated with ``ptr`` [L + 1]; m_r = n_used[r] in 1 .. n.
  Viterbi: V_0[j] = score[r0, j] for j < m_0.  Per step r -> r + 1 and per j < m_{r+1}: best = -inf, arg = 0; for i = 0 .. m_r - 1
  ascending cand = V[i] - g[r] * d2[r, i, j], replaced on strict cand > best (a NaN candidate never wins); V'[j] = score[r + 1, j] +
  best, back[r + 1, j] = arg.  The path ends at the first maximum of V over j < m_last (``log_score``) and is walked back.
  Marginals (scaled forward-backward): w = exp(score); alpha_0 = w_0 / s_0; u[j] = sum_i alpha[i] exp(-(g[r] d2[r, i, j])), i
  ascending; u <- w_{r+1} u; s_{r+1} = sum u; alpha' = u / s_{r+1}; beta_last = 1, beta_r[i] = sum_j exp(-(g[r] d2[r, i, j])) w_{r+1}[j]
  beta_{r+1}[j] / s_{r+1}; gamma = alpha beta normalised per sounding, 0 for the states >= m_r; log_partition = sum ln s.
Nothing outside the prefixes i < m_r, j < m_{r+1} of d2 is read, nor the entry of a sequence's last sounding.

``python -m geobipy_amd.sections <survey.npz> --depth Z1 [--from Z0] [--measure log] [--tau T | --fit-tau] [--length L] [--max-models n]
[--chains C] [--no-marginals] [--draws R [--seed N]] [--depth-axis N WIDTH [--percentiles P ...] [--exceed T ...]]`` writes
``<name>.sections.npz``.  There is no host fallback: ``cross_distance``, ``track``, ``draw``, ``sections`` and ``lateral_products``
refuse tensors that are not on the device.  ``survey.infer`` is not wired: its blocks cut across lines, so a lateral product is a step
after the run, like ``horizons.from_products``.  Left out on purpose: carrying a sequence across launches.  (Learning ``tau``, which
this list used to name, is ``fit_tau`` below; a ``score`` is no longer left to the caller alone: ``boreholes=`` makes one
from borehole logs.)  (The weighted re-binning by ``weight`` that this list used to name is
``lateral_products``; coupling across lines is ``spatial``.)

Across lines (gbp_section_propagate: csrc/gbp_section_graph.h).  ``neighbours`` joins every sounding to the next of
its line and to the nearest sounding of every other line within ``max_distance``; ``edge_distance`` gives D^2 per edge through
``cross_distance``; ``propagate`` runs synchronous sum-product message passing on that graph (``propagate_reference`` states the rule)
and returns *beliefs*: the marginals on a forest, a documented approximation on a graph with loops; ``spatial`` is all of it for an
ensemble, with the keys of ``sections`` that still have a meaning, and ``spatial_from_survey`` / ``from_survey(..., spatial=dict(
max_distance=...))`` / ``--spatial MAX_DISTANCE [--sweeps N] [--damping L]`` (``<name>.spatial.npz``) for a survey.  Left out on
purpose: tree-reweighted variants, wiring into ``survey.infer`` (learning ``tau`` is ``fit_tau_graph`` below).

The most probable section across lines (gbp_section_graph_path, gbp_section_graph_refine:
csrc/gbp_section_graph_path.h).  ``state`` of ``spatial`` is every sounding's most believed model taken alone; ``graph_path`` finds
one section for the whole graph: max-sum message passing in the log domain (``graph_path_reference`` states the rule, and the device
has its bits: there is no exp and no reordered sum), a decode that conditions level by level (``decode_levels``) so that equal modes
are never mixed, and coordinate ascent on the exact score (``refine``, ``sounding_colours``) from the decode and from any candidates
given, of which the most probable is kept.  Exact on a forest; on loops an approximation that is never below its candidates.
``spatial(..., path=True)`` adds ``path_state``, ``path_slot``, ``path_k`` / ``path_edges`` / ``path_sigma``, ``path_log_score``
beside ``state_log_score``, ``path_margin``, ``path_residual``, ``path_candidate_log_score``, ``path_chosen`` and
``path_edge_distance``; ``--spatial D --path [SWEEPS]`` writes them.  Left out on purpose: tree-reweighted variants, cluster moves.

Joint draws across lines (gbp_section_graph_draw: csrc/gbp_section_graph_draw.h).  ``graph_draw`` draws R joint
realisations of the whole graph by Gibbs sampling blocked by flight line (``graph_draw_reference`` states the rule, ``line_colours``
which lines one launch may draw together): from the line-alone start of ``draw``, every sweep redraws every line exactly from its
conditional given its neighbours' current states.  The stationary law is the exact joint, loops included; the realisations are
draws of it as far as ``sweeps`` sweeps have mixed, and 8 is a convention.  ``propagate(..., keep_kernel=True)`` hands its K on,
``spatial(..., draws=R, seed=N, draw_sweeps=T)`` adds ``draw_state``, ``draw_slot``, ``draw_log_score``, ``draw_share`` and
``draw_change_share``, and ``--spatial D --spatial-draws R [--seed N] [--draw-sweeps T]`` writes them.  Left out on purpose: the
filter on the matrix cores, cluster moves and tempering.  (Learning ``tau``: the pair potential exp(-g D^2) is not a normalised
transition, so ``log_partition`` alone grows monotonically as g -> 0; ``fit_tau`` below adds the normaliser.)  (Draws conditioned on boreholes, which this list used to name, are
``boreholes=`` below.)

Borehole logs (gbp_borehole_score: csrc/gbp_boreholes.h, through ``geobipy_amd.boreholes``).  ``sections(...,
boreholes=dict(logs=, max_distance=, surface=, classes=, class_floor=))`` and ``spatial(..., boreholes=...)`` attach every log to the
nearest sounding of every line within ``max_distance``, score every kept model of those soundings against the log and add that to
``score``: the path, the marginals or beliefs, the draws, and through ``weight`` and ``draw_slot`` the lateral products and bodies are
then conditioned on the logs.  They add ``borehole_score``, ``borehole_sounding``, ``borehole_index``, ``borehole_distance``,
``borehole_skipped`` and ``borehole_log_predictive``; ``--boreholes LOGS --borehole-distance D [--class-means M ... --class-scales S
...] [--class-floor F]`` does the same from the command line, with and without ``--spatial``, ``--draws`` and ``--bodies``.  Left out on
purpose: deviated wells, fitting a log's ``sd``, wiring into ``survey.infer``, feeding logs back into the sampler's prior.

Learning ``tau`` (gbp_section_evidence, gbp_section_graph_evidence: csrc/gbp_section_evidence.h).  The RMS difference
across a step is a scalar Gaussian of variance tau^2 dx / length, density sqrt(c g / pi) exp(-c g D^2) with g at a base tau0 and c =
(tau0 / tau)^2; up to a term that does not depend on tau the log evidence of c is log_partition(c) + rank / 2 ln c - sum_s ln sum_i
w_s[i], rank the number of soundings minus the number of connected pieces (along lines: the steps), and its derivative in lambda =
ln c is dlog_partition + rank / 2 with dlog_partition = -E[sum c g D^2]: at the fit the expected total cost is rank / 2.  ``evidence``
gives value and derivative for a ladder of tau (a factor sqrt 2 per rung) from one forward pass over ``d2`` per launch
(``evidence_reference`` and ``evidence_reference_ladder`` state the rule); ``graph_evidence`` the same for the survey graph through
the Bethe free energy of the messages ``propagate(..., keep_messages=True)`` hands on (``graph_terms``, ``graph_terms_reference``,
``graph_evidence_reference``, ``graph_rank``), with ``edge_energy``, the expected cost per edge; ``fit_tau`` / ``fit_tau_graph``
(``fit_tau_reference`` / ``fit_tau_graph_reference``) find the zero and its Laplace standard error, ``fit_ensemble`` and
``fit_from_survey`` do so for an ensemble and a survey, and ``--fit-tau [TAU_MAX [RUNGS]]`` runs the fit first, uses tau_hat for
everything else and stores ``fit_tau``, ``fit_tau_sd_log``, ``fit_tau_ladder`` and ``fit_log_evidence``.  ``tau`` stays 0.1 wherever
no fit is asked for.  Left out on purpose: learning ``slope`` and ``switch`` of ``horizons`` (the same tangent pass would do), a
``tau`` per line or per depth window, expected costs per step along lines (they need the backward pass), ``survey.infer``.

Connected bodies of the realisations (gbp_bodies_label: csrc/gbp_bodies.h, through ``geobipy_amd.bodies``).
``draw_bodies`` rasters the drawn models, on terrain resamples them onto one elevation axis, labels the connected bodies of the cells
with lo <= value <= hi and summarises them; ``sections(..., draws=R, bodies=dict(depth_edges=, lo=, hi=))`` and ``spatial(..., draws=R,
bodies=dict(...))`` add ``body_count``, ``body_largest_measure``, ``body_member_measure`` and ``body_largest_share``, and ``--bodies LO
HI --depth-axis N WIDTH`` with ``--draws R`` or ``--spatial D --spatial-draws R`` writes them.
"""
import numpy as np
import torch

from . import _args, _lib
from . import boreholes as _bh
from ._args import are_tensors, check_block, check_ensemble, check_int, first_max, host, on_device
from ._args import load_npz as load, save_npz as save  # noqa: F401  (this module's ``save`` and ``load``)
from .ensembles import Ensemble, check_chains, realisations
from .families import MAX_K, MAX_MODELS, check_window, distance_reference, used_rows

MAX_STATES = 1024
MAX_DRAWS = 65536
OUTPUT_SUFFIX = ".sections.npz"


def check_ptr(ptr, total, empty=False):
    """``ptr`` as int64 numpy [L + 1]: starts at 0, ends at ``total``, every sequence holds at least one sounding (``empty``: or none)."""
    return _args.check_ptr(ptr, total, "sections", empty)


def _default_ptr(ptr, total):
    """``ptr`` checked; None: one sequence of all the soundings (no sequence when there are none)."""
    if ptr is None:
        return np.array([0, total] if total else [0], dtype=np.int64)
    return check_ptr(ptr, total)


def _check_number(v, what, positive=True):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or (positive and not v > 0):
        raise ValueError("sections: %s must be a %s number" % (what, "positive finite" if positive else "finite"))
    return float(v)


# ---- which soundings follow which ---------------------------------------------------------------------------------------------------

def partners(ptr, n_used):
    """int32 [S] (numpy): the sounding that sounding s is paired with -- s + 1 within a sequence of ``ptr`` [L + 1] (None: one sequence),
    -1 at a sequence's end.  Sequences are cut at soundings with ``n_used`` == 0: such a sounding, and the one before it, get -1."""
    nu = host(n_used).reshape(-1)
    S = nu.size
    p = _default_ptr(ptr, S)
    out = np.arange(1, S + 1, dtype=np.int32)
    out[p[1:] - 1] = -1
    empty = nu <= 0
    out[empty] = -1
    out[:-1][empty[1:]] = -1
    return out


def pieces(ptr, n_used):
    """The chains of a launch: (keep int64 [T], piece_ptr int64 [P + 1], owner int64 [P]) -- the soundings with models in their order,
    the runs of them that ``partners`` connects as sequences over ``keep``, and the sequence of ``ptr`` every run belongs to."""
    nu = host(n_used).reshape(-1)
    p = _default_ptr(ptr, nu.size)
    partner = partners(p, nu)
    keep = np.flatnonzero(nu > 0).astype(np.int64)
    ends = np.flatnonzero(partner[keep] < 0)
    piece_ptr = np.concatenate([[0], ends + 1]).astype(np.int64)
    owner = (np.searchsorted(p, keep[piece_ptr[:-1]], side="right") - 1).astype(np.int64)
    return keep, piece_ptr, owner


# ---- the rules ----------------------------------------------------------------------------------------------------------------------

def cross_distance_reference(k, edges, sigma, rows, partner, z0, z1, measure="linear", dtype=np.float64, stored=False, squared=True):
    """The rule of ``cross_distance`` in numpy: ``k`` [S, n_slots], ``edges`` / ``sigma`` [S, n_slots, K], ``rows`` [S, n], ``partner``
    [S].  Returns D^2 (``squared``) or D [S, n, n] in ``dtype``: the slots of sounding s and of its partner are stacked into one
    sounding of 2 n_slots slots and the block [:n, n:] of ``families.distance_reference`` on the 2 n models is taken -- the same rule by
    construction.  A row outside the slots or an empty slot gives NaN in its row or column; a partner outside 0 .. S - 1 a slab of NaN."""
    k, edges, sigma, rows, partner = np.asarray(k), np.asarray(edges), np.asarray(sigma), np.asarray(rows), np.asarray(partner).reshape(-1)
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or edges.shape[:2] != k.shape or rows.ndim != 2 or rows.shape[0] != k.shape[0] \
            or partner.size != k.shape[0]:
        raise ValueError("cross_distance_reference: k [S, n_slots], edges and sigma [S, n_slots, K], rows [S, n], partner [S]")
    S, ns = k.shape
    n = rows.shape[1]
    out = np.full((S, n, n), np.nan, dtype=dtype)
    inside = lambda r: np.where((r >= 0) & (r < ns), r, -1).astype(np.int64)      # noqa: E731  (a row past the end must not name a partner's slot)
    for s in range(S):
        p = int(partner[s])
        if not 0 <= p < S:
            continue
        mine, theirs = inside(rows[s]), inside(rows[p])
        both = np.concatenate([mine, np.where(theirs >= 0, theirs + ns, -1)])
        D = distance_reference(np.concatenate([k[s], k[p]]), np.concatenate([edges[s], edges[p]]), np.concatenate([sigma[s], sigma[p]]), both, z0, z1,
                               measure=measure, dtype=dtype, stored=stored, squared=squared)
        out[s] = D[:n, n:]
    return out


def steps(x, y, tau=0.1, length=100.0, min_distance=1.0, ptr=None):
    """g float64 [S] (numpy) of the steps s -> s + 1 of soundings at ``x``, ``y`` (m): g[s] = length / (2 tau^2 max(dx_s, min_distance))
    with dx_s the horizontal distance.  The RMS difference in decades between neighbouring models is taken as a random walk of standard
    deviation ``tau`` per ``length`` metres: over dx its variance is tau^2 dx / length, and -g D^2 is the Gaussian log density of a
    difference D.  ``tau`` = 0.1 decades per 100 m and the floor of 1 m are a documented convention, not fitted numbers;
    on the planted line of the tests the path is the same for every tau in 0.05 .. 0.4.  The entry of a sequence's last sounding (of
    ``ptr``; default one sequence) is unused and holds length / (2 tau^2 min_distance)."""
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != y.size:
        raise ValueError("sections.steps: x and y must have one entry per sounding")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("sections.steps: x and y must be finite")
    tau, length, min_distance = _check_number(tau, "tau"), _check_number(length, "length"), _check_number(min_distance, "min_distance")
    S = x.size
    dx = np.zeros(S)
    if S > 1:
        dx[:-1] = np.hypot(np.diff(x), np.diff(y))
    if ptr is not None and S > 0:
        dx[check_ptr(ptr, S)[1:] - 1] = 0.0
    return length / (2.0 * tau * tau * np.maximum(dx, min_distance))


def _check_chain(ptr, score, g, d2, n_used, what, empty=False):
    """The host checks ``track``, ``draw`` and their references share; returns ptr (numpy), n_used (numpy int64)."""
    if d2.ndim != 3 or d2.shape[1] != d2.shape[2] or not 1 <= d2.shape[1] <= MAX_STATES:
        raise ValueError("%s: d2 [T, n, n] with 1 <= n <= %d" % (what, MAX_STATES))
    total, n = d2.shape[0], d2.shape[1]
    ptr = check_ptr(ptr, total, empty)
    nu = host(n_used).reshape(-1)
    if nu.size != total or nu.dtype.kind not in "iu":
        raise ValueError("%s: n_used must hold one integer per sounding" % what)
    if np.any(nu < 1) or np.any(nu > n):
        raise ValueError("%s: n_used must lie in 1 .. n (sequences are cut at soundings without models: sections.pieces)" % what)
    if np.size(g) != total:
        raise ValueError("%s: g must hold one entry per sounding" % what)
    if score is not None and tuple(score.shape) != (total, n):
        raise ValueError("%s: score must be [T, n]" % what)
    return ptr, nu.astype(np.int64)


def track_reference(ptr, score, g, d2, n_used, marginals=True, dtype=np.float64):
    """The rule of the module's docstring in numpy, evaluated in ``dtype`` (fp64: what the device is held to; np.longdouble: the
    yardstick of the rule's own rounding).  ``ptr`` [L + 1], ``score`` [T, n] or None (zeros), ``g`` [T], ``d2`` [T, n, n], ``n_used``
    [T] in 1 .. n.  Returns ``state`` int32 [T], ``log_score`` [L], and with ``marginals`` ``marginal`` [T, n], ``log_partition`` [L] and
    ``scale`` [T]."""
    ft = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.track_reference")
    total, n = d2.shape[0], d2.shape[1]
    score = (np.zeros((total, n)) if score is None else score).astype(ft)
    g = np.asarray(g, dtype=np.float64).reshape(-1).astype(ft)
    L = ptr.size - 1
    state, log_score = np.zeros(total, dtype=np.int32), np.zeros(L, dtype=ft)
    out = dict(state=state, log_score=log_score)
    if marginals:
        gamma, log_partition, scale = np.zeros((total, n), dtype=ft), np.zeros(L, dtype=ft), np.zeros(total, dtype=ft)
        out.update(marginal=gamma, log_partition=log_partition, scale=scale)
    for l in range(L):
        r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
        m = [int(v) for v in nu[r0:r0 + N]]
        cost = [g[r0 + s] * d2[r0 + s, :m[s], :m[s + 1]].astype(ft) for s in range(N - 1)]      # one multiply per entry, prefixes only
        # ---- Viterbi
        V = score[r0, :m[0]]
        back = [np.zeros(m[0], dtype=np.int64)]
        for s in range(N - 1):
            best, arg = np.full(m[s + 1], -np.inf, dtype=ft), np.zeros(m[s + 1], dtype=np.int64)
            with np.errstate(invalid="ignore"):
                for i in range(m[s]):                                        # i ascending
                    cand = V[i] - cost[s][i]
                    repl = cand > best                                       # strict: the first maximum stays, a NaN never wins
                    best, arg = np.where(repl, cand, best), np.where(repl, i, arg)
            V = score[r0 + s + 1, :m[s + 1]] + best
            back.append(arg)
        cur = first_max(V)
        log_score[l] = V[cur]
        for s in range(N - 1, -1, -1):
            state[r0 + s] = cur
            cur = int(back[s][cur])
        if not marginals:
            continue
        # ---- scaled forward-backward
        w = [np.exp(score[r0 + s, :m[s]]) for s in range(N)]
        E = [np.exp(-c) for c in cost]
        alpha, sc = [None] * N, np.zeros(N, dtype=ft)
        sc[0] = w[0].sum()
        alpha[0] = w[0] / sc[0]
        for s in range(N - 1):
            u = np.zeros(m[s + 1], dtype=ft)
            for i in range(m[s]):                                            # i ascending
                u = u + alpha[s][i] * E[s][i]
            u = w[s + 1] * u
            sc[s + 1] = u.sum()
            alpha[s + 1] = u / sc[s + 1]
        beta = np.ones(m[N - 1], dtype=ft)
        for s in range(N - 1, -1, -1):
            if s < N - 1:
                u = w[s + 1] * beta
                b = np.zeros(m[s], dtype=ft)
                for j in range(m[s + 1]):                                    # j ascending
                    b = b + E[s][:, j] * u[j]
                beta = b / sc[s + 1]
            gm = alpha[s] * beta
            gamma[r0 + s, :m[s]] = gm / gm.sum()
        scale[r0:r0 + N] = sc
        log_partition[l] = np.cumsum(np.log(sc))[-1]
    return out


# ---- learning tau: the evidence of the coupling and its derivative --------------------------------------------------

MAX_RUNGS = 8                       # the rungs of one launch
MAX_RUNG_STATES = 2048              # rungs * n of one launch: the filters and their tangents fill the LDS
FIT_TOLERANCE = 2e-3                # the bracket in lambda = ln c at which the refinement stops
FIT_EVALUATIONS = 12                # ... or this many single-rung evaluations


def evidence_reference(ptr, score, g, d2, n_used, T=1, dtype=np.float64):
    """The rule of gbp_section_evidence in numpy, evaluated in ``dtype``: ``log_partition`` and ``dlog_partition`` [T, L] of the chain
    of ``track_reference`` for the ladder of scales c_t = 2^t, t = 0 .. T - 1, of the step costs (``g`` already holds the lowest
    scale); the derivative is taken in lambda = ln c.  Arguments as ``track_reference`` takes them; prefixes only.

    Per sequence and rung t the normalised filter a_t and its tangent b_t = d a_t / d lambda.  Start: a = w_0 / sum w_0, b = 0,
    log Z = ln sum w_0, dlog Z = 0 (w = exp(score)).  Per step: cost_0 = g[r] * d2[r, i, j] (one multiply per entry), e_0 =
    exp(-cost_0) (one exp per entry); e_t = e_{t-1} * e_{t-1}, cost_t = cost_{t-1} + cost_{t-1} (exact); u_j = w_j sum_i a_t[i] e_t[i, j];
    u'_j = w_j sum_i (b_t[i] - a_t[i] cost_t[i, j]) e_t[i, j]; z = sum_j u_j, z' = sum_j u'_j; log Z += ln z, dlog Z += z' / z; a_t =
    u / z, b_t = u' / z - a_t (z' / z).  The sums are numpy's (``sum`` over an axis): their order is not part of the rule.  dlog Z is
    -E[sum c_t g D^2], the expected total cost of a section.  A sequence of one sounding has ln sum w_0 and 0.0; where a step's z
    underflows to 0 the rung is -inf or NaN from there on, and the rungs below it are not affected."""
    ft = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.evidence_reference", empty=True)
    T = check_int(T, 1, MAX_RUNGS, "sections.evidence_reference: T")
    total, n = d2.shape[0], d2.shape[1]
    score = (np.zeros((total, n)) if score is None else score).astype(ft)
    g = np.asarray(g, dtype=np.float64).reshape(-1).astype(ft)
    L = ptr.size - 1
    log_z, dlog_z = np.zeros((T, L), dtype=ft), np.zeros((T, L), dtype=ft)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for l in range(L):
            r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
            if N <= 0:
                continue
            m = [int(v) for v in nu[r0:r0 + N]]
            w = np.exp(score[r0, :m[0]])
            s = w.sum()
            a, b = [w / s for _ in range(T)], [np.zeros(m[0], dtype=ft) for _ in range(T)]
            log_z[:, l] = np.log(s)
            for st in range(N - 1):
                r = r0 + st
                cost = g[r] * d2[r, :m[st], :m[st + 1]].astype(ft)
                e = np.exp(-cost)
                w = np.exp(score[r + 1, :m[st + 1]])
                for t in range(T):
                    if t:
                        e, cost = e * e, cost + cost
                    u = w * (a[t][:, None] * e).sum(axis=0)
                    up = w * ((b[t][:, None] - a[t][:, None] * cost) * e).sum(axis=0)
                    z, zp = u.sum(), up.sum()
                    log_z[t, l] += np.log(z)
                    dlog_z[t, l] += zp / z
                    a[t] = u / z
                    b[t] = up / z - a[t] * (zp / z)
    return dict(log_partition=log_z, dlog_partition=dlog_z)


def ladder_launches(n, rungs):
    """[(first rung, rungs)] of the launches a ladder of ``rungs`` rungs over ``n`` states takes: at most 8 rungs and rungs * n <= 2048
    per launch.  Every launch's lowest rung takes its own exp; the rungs above it are squarings."""
    per = max(1, min(MAX_RUNGS, MAX_RUNG_STATES // max(int(n), 1)))
    return [(t, min(per, rungs - t)) for t in range(0, rungs, per)]


def _check_ladder(tau0, rungs, scale, what):
    return _check_number(tau0, "tau0"), check_int(rungs, 1, 64, "%s: rungs" % what), _check_number(scale, "scale")


def _log_weights(score, nu):
    """float64 [T] (numpy): ln sum_i w_s[i] over the prefix of every sounding (``score`` numpy [T, n] or None: ln m_s)."""
    if score is None:
        return np.log(nu.astype(np.float64))
    out = np.empty(nu.size)
    for s in range(nu.size):
        v = np.asarray(score[s, :nu[s]], dtype=np.float64)
        top = v.max()
        out[s] = top + np.log(np.exp(v - top).sum()) if np.isfinite(top) else top
    return out


def _ladder_result(log_z, dlog_z, ptr, log_w, tau0, scale):
    """What ``evidence`` and ``evidence_reference_ladder`` return, from log Z and dlog Z [T, L] (numpy float64)."""
    T = log_z.shape[0]
    c = scale * 2.0 ** np.arange(T)
    rank = (np.diff(ptr) - 1).clip(min=0).astype(np.int64)
    base = np.array([log_w[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])], dtype=np.float64)
    return dict(tau=tau0 / np.sqrt(c), scale=c, rank=rank, log_partition=log_z, dlog_partition=dlog_z,
                log_evidence=log_z + 0.5 * rank[None, :] * np.log(c)[:, None] - base[None, :])


def evidence_reference_ladder(d2, g, ptr, n_used, score=None, tau0=0.1, rungs=1, scale=1.0, dtype=np.float64):
    """The rule of ``evidence``: ``evidence_reference`` launch by launch as ``ladder_launches`` splits the ladder, every launch's ``g``
    multiplied by its lowest scale (one multiply per step, in float64).  numpy arrays throughout; returns what ``evidence`` returns."""
    tau0, rungs, scale = _check_ladder(tau0, rungs, scale, "sections.evidence_reference_ladder")
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.evidence_reference_ladder", empty=True)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    parts = [evidence_reference(ptr, score, g * (scale * 2.0 ** t0), d2, nu, T=T, dtype=dtype) for t0, T in ladder_launches(d2.shape[1], rungs)]
    log_z, dlog_z = (np.concatenate([p[name] for p in parts]).astype(np.float64) for name in ("log_partition", "dlog_partition"))
    return _ladder_result(log_z, dlog_z, ptr, _log_weights(score, nu), tau0, scale)


def _fit(evaluate, tau_max, rungs):
    """The fit ``fit_tau`` and ``fit_tau_reference`` share.  ``evaluate(scale, rungs)`` gives the ladder result of ``evidence`` (numpy)
    with ``g`` at ``tau_max``.  f(lambda) = sum_l dlog_partition + rank / 2 is the derivative of the pooled log evidence in lambda =
    ln c, c = (tau_max / tau)^2: positive where the walk is too loose, negative where it is too stiff."""
    lad = evaluate(1.0, rungs)
    rank = int(lad["rank"].sum())
    lam = np.log(lad["scale"])
    f = lad["dlog_partition"].sum(axis=1) + 0.5 * rank
    pooled = lad["log_evidence"].sum(axis=1)
    out = dict(tau_ladder=lad["tau"], log_evidence=pooled, log_evidence_sequence=lad["log_evidence"], expected_cost=-lad["dlog_partition"].sum(axis=1),
               rank=rank, bracketed=False, bracket=(-1, -1), tau_sd_log=float("nan"), evaluations=0)
    out.update({name: lad[name] for name in ("residual", "edge_energy") if name in lad})      # (the graph's ladder has them)
    ok = np.flatnonzero(np.isfinite(f) & np.isfinite(pooled))                # non-finite rungs are skipped
    pair = next(((int(a), int(b)) for a, b in zip(ok[:-1], ok[1:]) if f[a] > 0.0 >= f[b]), None)
    if pair is None:
        # no sign change: the ladder's end on the side the derivative points to (its last finite rung where f > 0 throughout)
        end = (ok[-1] if f[ok[-1]] > 0.0 else ok[0]) if ok.size else rungs - 1
        out["tau"] = float(lad["tau"][end])
        return out
    lo, hi, f_lo, f_hi = float(lam[pair[0]]), float(lam[pair[1]]), float(f[pair[0]]), float(f[pair[1]])
    n_eval = 0
    while hi - lo >= FIT_TOLERANCE and n_eval < FIT_EVALUATIONS:              # bisection: every evaluation halves the bracket
        mid = 0.5 * (lo + hi)
        one = evaluate(float(np.exp(mid)), 1)
        f_mid = float(one["dlog_partition"].sum() + 0.5 * rank)
        n_eval += 1
        if not np.isfinite(f_mid):
            break
        if f_mid > 0.0:
            lo, f_lo = mid, f_mid
        else:
            hi, f_hi = mid, f_mid
    slope = (f_hi - f_lo) / (hi - lo)                                         # f' < 0: the curvature of the log evidence in lambda
    root = lo - f_lo / slope                                                  # the secant's zero within the last bracket
    out.update(tau=float(tau_max * np.exp(-0.5 * root)), tau_sd_log=float(0.5 / np.sqrt(-slope)), bracketed=True, bracket=pair, evaluations=n_eval)
    return out


def _check_fit(tau_max, rungs, what):
    return _check_number(tau_max, "tau_max"), check_int(rungs, 2, 64, "%s: rungs" % what)


def fit_tau_reference(d2, g, ptr, n_used, score=None, tau0=0.1, tau_max=0.8, rungs=11, dtype=np.float64):
    """``fit_tau`` on the rules (``evidence_reference_ladder``), numpy arrays throughout."""
    tau_max, rungs = _check_fit(tau_max, rungs, "sections.fit_tau_reference")
    tau0 = _check_ladder(tau0, 1, 1.0, "sections.fit_tau_reference")[0]
    g_max = np.asarray(host(g), dtype=np.float64).reshape(-1) * (tau0 / tau_max) ** 2
    return _fit(lambda scale, T: evidence_reference_ladder(d2, g_max, ptr, n_used, score=score, tau0=tau_max, rungs=T, scale=scale, dtype=dtype),
                tau_max, rungs)


# ---- joint draws: the rule ----------------------------------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("sections: seed must be an integer in 0 .. 2^64 - 1")
    return int(seed)


def _check_row_key(row_key, total, what):
    """``row_key`` as int64 numpy [T]; None: the row index."""
    if row_key is None:
        return np.arange(total, dtype=np.int64)
    key = host(row_key)
    if key.shape != (total,) or key.dtype.kind not in "iu":
        raise ValueError("%s: row_key must hold one integer per sounding" % what)
    return key.astype(np.int64)


def philox_uniform(seed, draw, row_key, sweep=0):
    """The uniform of a draw, float64 in [0, 1), vectorised over ``draw`` and ``row_key`` (broadcast against each other): u53(x, y) of
    the Philox4x32-10 block with key ``seed`` (uint64: low word, high word) and counter (draw, row_key & 0xFFFFFFFF, row_key >> 32,
    sweep) -- the generator and the 53-bit uniform of the sampler (csrc/gbp_philox.h), counter layout of the section draws (DESIGN.md
    3.26); ``sweep`` is 0 but for the sweeps of the draws across lines."""
    seed = _check_seed(seed)
    sweep = check_int(sweep, 0, 2 ** 32 - 1, "sections: sweep")
    c0, key = np.broadcast_arrays(np.asarray(draw, dtype=np.int64).astype(np.uint64) & _M32, np.asarray(row_key, dtype=np.int64).astype(np.uint64))
    c1, c2, c3 = key & _M32, key >> _S32, np.full(key.shape, sweep, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> _S32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return ((c0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (c1 >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def draw_reference(ptr, score, g, d2, n_used, n_draws, seed=0, row_key=None, dtype=np.float64):
    """The rule of ``draw`` in numpy, evaluated in ``dtype``: joint draws of whole sections from the chain of the module's docstring
    by forward filtering and backward sampling.  The inputs of ``track_reference`` (a sequence of ``ptr`` may be empty here), ``n_draws``
    = R in 1 .. 65536, ``seed`` (uint64) and ``row_key`` int64 [T] (None: the row index).

    Filter, per sequence: the forward pass of ``track_reference``, word for word -- w_s = exp(score), alpha_0 = w_0 / sum w_0, u[j] =
    sum_i alpha_s[i] exp(-(g_s d2[s, i, j])) with i ascending and u = u + a * e, alpha_{s+1} = (w_{s+1} u) / sum.
    Draws: realisation rho walks s = N - 1 .. 0.  Over i < m_s the weights are W[i] = alpha_s[i] at the last sounding and alpha_s[i] *
    exp(-(g_s * d2[s, i, j])) elsewhere, j the state just drawn under s + 1; c = cumsum(W), sequential with i ascending; thr = u *
    c[m_s - 1]; pick = min(#{i : c[i] <= thr}, m_s - 1).  A state of weight 0 is never the first to pass thr, so it is never drawn; with
    a NaN total no comparison holds and the pick is 0.  u = ``philox_uniform(seed, rho, row_key[s])``: a draw depends on the seed, the
    realisation and the sounding's key -- not on R, on the grouping of sequences into calls, or on a launch shape.

    Returns ``draw_state`` int32 [R, T], ``filtered`` [T, n] (alpha, 0.0 for the states >= m_s) and ``margin`` [R, T] = min_i |c[i] -
    thr| / c[m_s - 1]: how close the draw came to another outcome (a device whose exp differs in the last bit may decide a draw with a
    margin of a few ulp the other way)."""
    ft = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.draw_reference", empty=True)
    R = check_int(n_draws, 1, MAX_DRAWS, "sections.draw_reference: n_draws")
    total, n = d2.shape[0], d2.shape[1]
    key = _check_row_key(row_key, total, "sections.draw_reference")
    seed = _check_seed(seed)
    score = (np.zeros((total, n)) if score is None else score).astype(ft)
    g = np.asarray(g, dtype=np.float64).reshape(-1).astype(ft)
    rho = np.arange(R, dtype=np.int64)
    draw_state, filtered, margin = np.zeros((R, total), dtype=np.int32), np.zeros((total, n), dtype=ft), np.zeros((R, total), dtype=ft)
    for l in range(ptr.size - 1):
        r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
        if N == 0:
            continue
        m = [int(v) for v in nu[r0:r0 + N]]
        E = [np.exp(-(g[r0 + s] * d2[r0 + s, :m[s], :m[s + 1]].astype(ft))) for s in range(N - 1)]      # prefixes only
        w = [np.exp(score[r0 + s, :m[s]]) for s in range(N)]
        alpha = [None] * N
        alpha[0] = w[0] / w[0].sum()
        for s in range(N - 1):
            u = np.zeros(m[s + 1], dtype=ft)
            for i in range(m[s]):                                            # i ascending
                u = u + alpha[s][i] * E[s][i]
            u = w[s + 1] * u
            alpha[s + 1] = u / u.sum()
        j = None
        for s in range(N - 1, -1, -1):
            filtered[r0 + s, :m[s]] = alpha[s]
            W = np.broadcast_to(alpha[s][None, :], (R, m[s])) if s == N - 1 else alpha[s][None, :] * E[s][:, j].T
            c = np.cumsum(W, axis=1, dtype=ft)                               # sequential, i ascending
            thr = philox_uniform(seed, rho, key[r0 + s]).astype(ft) * c[:, -1]
            with np.errstate(invalid="ignore", divide="ignore"):
                j = np.minimum((c <= thr[:, None]).sum(axis=1), m[s] - 1)
                margin[:, r0 + s] = np.abs(c - thr[:, None]).min(axis=1) / c[:, -1]
            draw_state[:, r0 + s] = j
    return dict(draw_state=draw_state, filtered=filtered, margin=margin)


def exceedance_area_reference(k, edges, sigma, x, y, ptr, threshold, z0, z1, above=True):
    """The rule of ``exceedance_area`` in numpy loops: [R, L] in m^2."""
    k, edges, sigma = np.asarray(k), np.asarray(edges, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    R, S = k.shape
    p = _default_ptr(ptr, S)
    width = section_widths(x, y, p)
    out = np.zeros((R, p.size - 1))
    for l in range(p.size - 1):
        for r in range(R):
            area = 0.0
            for s in range(int(p[l]), int(p[l + 1])):
                thick = 0.0
                for q in range(int(k[r, s])):
                    top, bottom = (0.0 if q == 0 else edges[r, s, q - 1]), (edges[r, s, q] if q < k[r, s] - 1 else np.inf)
                    if (sigma[r, s, q] >= threshold) if above else (sigma[r, s, q] < threshold):
                        thick = thick + max(0.0, min(bottom, z1) - max(top, z0))
                area = area + width[s] * thick
            out[r, l] = area
    return out


# ---- the entries --------------------------------------------------------------------------------------------------------------------

def cross_distance(ens, rows, partner, z0, z1, measure="linear", squared=True, log10=True, block=None):
    """D^2 (``squared``; else D) f64 [S, n, n] on the device: entry [s, i, j] is the distance of ``families.distance`` between model
    ``rows[s, i]`` of sounding s and model ``rows[partner[s], j]`` of sounding ``partner[s]`` (``rows`` int32 [S, n] on the device;
    ``partner`` int32 [S], what ``partners`` gives: numpy or torch) over the window [z0, z1].  An absent model gives NaN in its row or
    column, a partner outside 0 .. S - 1 a slab of NaN (``cross_distance_reference`` states the rule).  ``block``: soundings per launch
    (None: one launch unless it would exceed 2^32 - 1 threads); a block brings the partners outside it along, the bits are the same.
    One kernel (gbp_ensemble_cross_distance)."""
    entry = "gbp_ensemble_cross_distance"
    are_tensors((ens.k, ens.edges, ens.sigma, rows), "sections", "cross_distance", entry)
    k, edges, sigma, S, ns, K = check_ensemble(ens, batch="S", rows=rows, what="cross_distance", max_rows=MAX_MODELS)
    if ns < 1 or not 1 <= K <= MAX_K:
        raise ValueError("ensemble: at least one slot and K in [1, %d]" % MAX_K)
    pn = host(partner)
    if pn.shape != (S,) or pn.dtype.kind not in "iu":
        raise ValueError("cross_distance: partner must hold one integer per sounding")
    z0, z1, log = check_window(z0, z1, measure)
    check_block(block, "cross_distance")
    on_device((k, edges, sigma, rows), "sections", "cross_distance", entry)
    rows, dev = rows.contiguous(), k.device
    n = rows.shape[1]
    out = torch.empty((S, n, n), dtype=torch.float64, device=dev)
    if S == 0:
        return out
    tiles = (n + 15) // 16
    step = (2 ** 32 - 1) // (256 * tiles * tiles) if block is None else int(block)      # soundings one launch takes: 256 threads per tile

    def launch(k_, e_, s_, rows_, partner_, out_):
        p_ = torch.as_tensor(np.ascontiguousarray(partner_, dtype=np.int32)).to(dev)
        _lib.call(entry, dev, k_.shape[0], ns, K, k_, e_, s_, n, rows_, p_, z0, z1, log, int(bool(log10)), int(bool(squared)), out_)

    if S <= step:
        launch(k, edges, sigma, rows, pn, out)
        return out
    for b0 in range(0, S, step):
        b1 = min(S, b0 + step)
        p = pn[b0:b1].astype(np.int64)
        valid = (p >= 0) & (p < S)
        extra = np.unique(p[valid & ((p < b0) | (p >= b1))])                  # the partners outside the block come along, unpaired
        local = np.where(valid, np.where((p >= b0) & (p < b1), p - b0, (b1 - b0) + np.searchsorted(extra, p)), -1)
        idx = torch.as_tensor(np.concatenate([np.arange(b0, b1), extra])).to(dev)
        part = torch.empty((idx.numel(), n, n), dtype=torch.float64, device=dev)
        launch(k[idx], edges[idx], sigma[idx], rows[idx], np.concatenate([local, np.full(extra.size, -1)]), part)
        out[b0:b1] = part[:b1 - b0]
    return out


def track(d2, g, ptr, n_used, score=None, marginals=True):
    """The most probable path and the smoothed marginals of the chain of the module's docstring (gbp_section_track): ``d2`` f64
    [T, n, n] on the device (what ``cross_distance`` gives for soundings in sequence order), ``g`` [T] (``steps``; host or device),
    ``ptr`` [L + 1] (host), ``n_used`` [T] in 1 .. n (host or device), ``score`` f64 [T, n] on the device or None: zeros -- the kept
    models are equally weighted samples.  Returns on the device ``state`` int32 [T], ``log_score`` [L], and with ``marginals``
    ``marginal`` [T, n], ``log_partition`` [L] and ``scale`` [T]."""
    entry = "gbp_section_track"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "track", entry)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.track")
    if d2.dtype != torch.float64 or (score is not None and score.dtype != torch.float64):
        raise TypeError("sections.track: d2 and score are float64")
    on_device((d2,) + (() if score is None else (score,)), "sections", "track", entry)
    dev = d2.device
    total, n = d2.shape[0], d2.shape[1]
    L = ptr.size - 1
    f64 = dict(dtype=torch.float64, device=dev)
    d2 = d2.contiguous()
    score = torch.zeros((total, n), **f64) if score is None else score.contiguous()
    t_ptr = torch.as_tensor(ptr, dtype=torch.int64).to(dev)
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev) if not torch.is_tensor(g) else g.to(dev, torch.float64).reshape(-1).contiguous()
    t_nu = torch.as_tensor(nu.astype(np.int32)).to(dev)
    back = torch.empty((total, n), dtype=torch.int16, device=dev)
    out = dict(state=torch.empty(total, dtype=torch.int32, device=dev), log_score=torch.empty(L, **f64))
    if marginals:
        out.update(marginal=torch.empty((total, n), **f64), log_partition=torch.empty(L, **f64), scale=torch.empty(total, **f64))
    if L > 0:
        _lib.call(entry, dev, L, t_ptr, total, n, t_nu, score, t_g, d2, back, out["state"], out["log_score"], out.get("marginal"),
                  out.get("log_partition"), out.get("scale"))
    return out


def evidence(d2, g, ptr, n_used, score=None, tau0=0.1, rungs=1, scale=1.0):
    """The evidence of the coupling for a ladder of ``rungs`` values of tau, and its exact derivative (gbp_section_evidence;
    ``evidence_reference_ladder`` states the rule).  ``d2``, ``g``, ``ptr``, ``n_used``, ``score`` as ``track`` takes
    them (a sequence of ``ptr`` may be empty); ``g`` is what ``steps`` gives for ``tau0``.  Rung t scales the step costs by c_t =
    ``scale`` 2^t, that is tau_t = ``tau0`` / sqrt(c_t): tau falls by sqrt 2 per rung.  One forward pass over ``d2`` serves up to 8 rungs
    with rungs * n <= 2048; a longer ladder takes further launches (``ladder_launches``).  Returns numpy arrays: ``tau`` and ``scale``
    [rungs], ``rank`` int64 [L] (the steps of every sequence), ``log_partition`` and ``dlog_partition`` [rungs, L] (the derivative in
    lambda = ln c: minus the expected total cost of a section) and ``log_evidence`` [rungs, L] = log_partition + rank / 2 ln c - sum_s
    ln sum_i w_s[i], the log evidence of tau up to a term that does not depend on it."""
    entry = "gbp_section_evidence"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "evidence", entry)
    g = host(g).reshape(-1).astype(np.float64)                               # (every launch scales it on the host)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.evidence", empty=True)
    tau0, rungs, scale = _check_ladder(tau0, rungs, scale, "sections.evidence")
    if d2.dtype != torch.float64 or (score is not None and score.dtype != torch.float64):
        raise TypeError("sections.evidence: d2 and score are float64")
    on_device((d2,) + (() if score is None else (score,)), "sections", "evidence", entry)
    dev = d2.device
    total, n = d2.shape[0], d2.shape[1]
    L = ptr.size - 1
    f64 = dict(dtype=torch.float64, device=dev)
    d2 = d2.contiguous()
    log_w = _log_weights(None if score is None else score.cpu().numpy(), nu)
    score = torch.zeros((total, n), **f64) if score is None else score.contiguous()
    t_ptr = torch.as_tensor(ptr, dtype=torch.int64).to(dev)
    t_nu = torch.as_tensor(nu.astype(np.int32)).to(dev)
    log_z, dlog_z = torch.zeros((rungs, L), **f64), torch.zeros((rungs, L), **f64)
    if L > 0:
        for t0, T in ladder_launches(n, rungs):
            t_g = torch.as_tensor(g * (scale * 2.0 ** t0)).to(dev)          # the launch's lowest scale, one multiply per step
            _lib.call(entry, dev, L, t_ptr, total, n, t_nu, score, t_g, d2, T, log_z[t0:t0 + T], dlog_z[t0:t0 + T])
    return _ladder_result(log_z.cpu().numpy(), dlog_z.cpu().numpy(), ptr, log_w, tau0, scale)


def fit_tau(d2, g, ptr, n_used, score=None, tau0=0.1, tau_max=0.8, rungs=11):
    """The lateral coupling tau learnt from the sections themselves: the zero of the pooled log evidence's derivative
    f(lambda) = sum_l dlog_partition + rank / 2 -- equipartition: the expected total cost of a section equals half the number of
    steps.  Arguments as ``evidence`` takes them, ``g`` at ``tau0``.  A ladder of ``rungs`` values from ``tau_max`` downward by sqrt 2
    (0.8 .. 0.025 by default) is evaluated in one pass per launch; the first sign change of f among its finite rungs is refined by
    bisection with single-rung launches until the bracket in lambda is below 2e-3 or 12 evaluations have been made; the zero is the
    secant's within the last bracket.  Returns ``tau``, ``tau_sd_log`` = 0.5 / sqrt(-f') from that bracket's slope (the Laplace
    standard error of ln tau), ``tau_ladder`` [rungs], ``log_evidence`` [rungs] pooled and ``log_evidence_sequence`` [rungs, L],
    ``expected_cost`` [rungs], ``rank``, ``bracketed``, ``bracket`` (the two rungs, (-1, -1) without) and ``evaluations``.  Where f
    does not change sign ``bracketed`` is False, ``tau`` is the ladder's end on the side f points to and ``tau_sd_log`` is NaN."""
    tau_max, rungs = _check_fit(tau_max, rungs, "sections.fit_tau")
    tau0 = _check_ladder(tau0, 1, 1.0, "sections.fit_tau")[0]
    g_max = host(g).reshape(-1).astype(np.float64) * (tau0 / tau_max) ** 2
    return _fit(lambda scale, T: evidence(d2, g_max, ptr, n_used, score=score, tau0=tau_max, rungs=T, scale=scale), tau_max, rungs)


def draw(d2, g, ptr, n_used, n_draws, seed=0, score=None, row_key=None):
    """Joint draws of whole sections from the chain of ``track`` by forward filtering and backward sampling (gbp_section_draw;
    ``draw_reference`` states the rule): ``d2``, ``g``, ``ptr``, ``n_used``, ``score`` as ``track`` takes them (a sequence of ``ptr``
    may be empty), ``n_draws`` = R in 1 .. 65536, ``seed`` a uint64, ``row_key`` int64 [T] (host or device; None: the row index) -- the
    uniform of realisation rho under a sounding is ``philox_uniform(seed, rho, row_key)``, so soundings keep their draws however they
    are grouped into calls.  Returns on the device ``draw_state`` int32 [R, T] and ``filtered`` [T, n]."""
    entry = "gbp_section_draw"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "draw", entry)
    ptr, nu = _check_chain(ptr, score, g, d2, n_used, "sections.draw", empty=True)
    R = check_int(n_draws, 1, MAX_DRAWS, "sections.draw: n_draws")
    seed = _check_seed(seed)
    if d2.dtype != torch.float64 or (score is not None and score.dtype != torch.float64):
        raise TypeError("sections.draw: d2 and score are float64")
    total, n = d2.shape[0], d2.shape[1]
    key = None if row_key is None else _check_row_key(row_key, total, "sections.draw")
    on_device((d2,) + (() if score is None else (score,)), "sections", "draw", entry)
    dev = d2.device
    L = ptr.size - 1
    f64 = dict(dtype=torch.float64, device=dev)
    d2 = d2.contiguous()
    score = torch.zeros((total, n), **f64) if score is None else score.contiguous()
    t_ptr = torch.as_tensor(ptr, dtype=torch.int64).to(dev)
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev) if not torch.is_tensor(g) else g.to(dev, torch.float64).reshape(-1).contiguous()
    t_nu = torch.as_tensor(nu.astype(np.int32)).to(dev)
    t_key = None if key is None else torch.as_tensor(key).to(dev)
    scale = torch.empty(total, **f64)
    out = dict(draw_state=torch.empty((R, total), dtype=torch.int32, device=dev), filtered=torch.empty((total, n), **f64))
    if L > 0 and total > 0:
        _lib.call(entry, dev, L, t_ptr, total, n, t_nu, score, t_g, d2, t_key, seed, R, out["filtered"], scale, out["draw_state"])
    return out


def _run_sums(terms, piece_ptr):
    """[R, P]: the sums of ``terms`` [R, T] over the runs of ``piece_ptr`` [P + 1], one reduction per run -- the shape of a run alone
    decides the order of its sum, not what else shares the launch."""
    out = torch.zeros((terms.shape[0], len(piece_ptr) - 1), dtype=terms.dtype, device=terms.device)
    for q in range(len(piece_ptr) - 1):
        out[:, q] = terms[:, int(piece_ptr[q]):int(piece_ptr[q + 1])].sum(dim=1)
    return out


def sections(ens, x, y, z1, z0=0.0, measure="linear", ptr=None, chains=1, max_models=128, tau=0.1, length=100.0, min_distance=1.0, score=None,
             marginals=True, budget_bytes=4 << 30, draws=0, seed=0, products=None, bodies=None, boreholes=None):
    """One kept model per sounding, chosen jointly along every sequence of ``ptr`` [L + 1] (None: one sequence) for the ensemble
    ``ens`` of soundings at ``x``, ``y`` [S] (host; m) over the depth window [z0, z1]: ``families.used_rows`` (``chains``,
    ``max_models`` <= 1024), ``cross_distance`` (squared), ``steps`` (``tau``, ``length``, ``min_distance``), ``track`` and a gather.
    ``score`` f64 [S, n] on the device: a log weight per used model (None: equal weights).  Sequences are cut at soundings without
    models.  Whole sequences are grouped into launches whose d2 stays under ``budget_bytes``; a single sequence that does not fit is
    refused (lower ``max_models`` or raise ``budget_bytes``): no state is carried between pieces.

    Returns, on the device: ``state`` int32 [S] (the position in ``rows``; -1: no models), ``slot`` int32 [S] (the ensemble slot; -1),
    ``rows`` int32 [S, n], ``n_used`` int32 [S], ``section_k`` int32 [S] (0: none), ``section_edges`` / ``section_sigma`` f64 [S, K]
    (bit copies of the chosen slots; NaN: none), ``step_distance`` f64 [S] (D in decades between the chosen models of s and s + 1; NaN at
    the end of a run), ``log_score`` f64 [L] (the sum over the sequence's runs; 0 for a sequence without models); with ``marginals``
    ``weight`` f64 [S, n] (the smoothed marginal of every used model; NaN: no models), ``chosen_weight`` [S], ``n_effective`` [S] =
    1 / sum w^2 (between 1 and n_used: how strongly the neighbours re-weight the sounding's samples) and ``log_partition`` [L].

    ``draws`` = R > 0 adds R joint realisations of every sequence from the chain's posterior (``draw`` with ``seed``; the key of a
    sounding is its index in the survey, so ``budget_bytes`` cannot change a draw): ``draw_state`` int32 [R, S] (the position in
    ``rows``; -1: no models), ``draw_slot`` int32 [R, S] (the ensemble slot; -1) and ``draw_log_score`` f64 [R, L] = sum score - sum g
    d2 along the drawn path, summed over a cut sequence's runs: on the scale of ``log_score``, so that ``draw_log_score -
    log_partition`` is the path's log probability.  ``draw_models`` gathers the models.

    ``products`` = dict(depth_edges=, percentiles=, thresholds=) adds what ``lateral_products`` returns for this result: the weighted
    mean, sd, percentiles and exceedance probabilities of every sounding's models under ``weight`` on a depth axis (it needs
    ``marginals``).  Without it the result is what it was, bit for bit.

    ``bodies`` = dict(depth_edges=, lo=, hi=, ...) (the keywords of ``draw_bodies`` but the geometry; it needs ``draws``) adds the
    connected bodies of the realisations along every sequence: ``body_count`` int64 [R, L], ``body_largest_measure`` /
    ``body_member_measure`` f64 [R, L] (m^2 under the default widths) and ``body_largest_share`` f64 [S, C], the share of realisations
    in which the cell belongs to the largest body of its sequence.  With None every other output keeps its bits.

    ``boreholes`` = dict(logs=, max_distance=, surface=None, classes=None, class_floor=1e-6) conditions everything above on borehole
    logs (``geobipy_amd.boreholes``): every log is attached to the nearest sounding with models of every sequence within
    ``max_distance`` (``boreholes.attach`` with this call's ``tau`` and ``length``), ``boreholes.score`` turns it into a log weight per
    kept model, and that is added to ``score`` -- so the path, the marginals, the draws and through ``weight`` and ``draw_slot`` the
    products and bodies all see it.  Adds ``borehole_score`` f64 [S, n], ``borehole_sounding`` / ``borehole_index`` int32 [A],
    ``borehole_distance`` f64 [A], ``borehole_skipped`` int32 [A] and, with ``marginals``, ``borehole_log_predictive`` f64 [A] under the
    result's own ``weight``.  With None every other output keeps its bits."""
    z0, z1, _ = check_window(z0, z1, measure)
    if boreholes is not None:
        boreholes = _bh.check_options(boreholes, "sections")
    if products is not None:
        products = check_products(products)
        if not marginals:
            raise ValueError("sections: products are weighted by the smoothed marginals; they need marginals=True")
    if bodies is not None:
        bodies = check_bodies(bodies, "sections")
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    are_tensors((k, edges, sigma), "sections", "sections", "gbp_ensemble_cross_distance")
    if k.ndim != 2 or edges.ndim != 3:
        raise ValueError("ensemble: k [S, n_slots], edges and sigma [S, n_slots, K]")
    C = check_chains(chains, k.shape[1])
    max_models = check_int(max_models, 1, MAX_STATES, "max_models")
    budget_bytes = check_int(budget_bytes, 1, 2 ** 62, "budget_bytes")
    R, seed = check_int(draws, 0, MAX_DRAWS, "draws"), _check_seed(seed)
    if bodies is not None and not R:
        raise ValueError("sections: bodies are those of joint realisations; they need draws >= 1")
    S, K = k.shape[0], edges.shape[2]
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != S or y.size != S:
        raise ValueError("sections: x and y must hold one entry per sounding (%d)" % S)
    p = _default_ptr(ptr, S)
    g = steps(x, y, tau, length, min_distance, p)
    rows, n_used, _ = used_rows(ens, chains=C, max_models=max_models)
    n = rows.shape[1]
    if score is not None:
        are_tensors((score,), "sections", "sections", "gbp_section_track")
        if tuple(score.shape) != (S, n) or score.dtype != torch.float64:
            raise ValueError("sections: score must be float64 [S, n] with n = %d, the width of used_rows" % n)
    dev, L = k.device, p.size - 1
    keep, piece_ptr, owner = pieces(p, n_used)
    slab = n * n * 8
    longest = int(np.diff(piece_ptr).max(initial=0))
    if longest * slab > budget_bytes:
        raise ValueError("sections: a sequence of %d soundings with %d models each needs %d bytes of distances, more than budget_bytes = %d; lower "
                         "max_models or raise budget_bytes (no state is carried between pieces of a sequence)" % (longest, n, longest * slab, budget_bytes))
    on_device((k, edges, sigma) + (() if score is None else (score,)), "sections", "sections", "gbp_ensemble_cross_distance")
    if boreholes is not None:
        b_score, b_att, b_part, b_skipped = _bh.section_score(ens, rows, n_used, x, y, p, boreholes, tau, length)
        score = b_score if score is None else score + b_score
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    nan = float("nan")
    state = torch.full((S,), -1, **i32)
    step_distance = torch.full((S,), nan, **f64)
    log_score = torch.zeros(L, **f64)
    weight = torch.full((S, n), nan, **f64) if marginals else None
    log_partition = torch.zeros(L, **f64) if marginals else None
    draw_state = torch.full((R, S), -1, **i32) if R else None
    draw_log_score = torch.zeros((R, L), **f64) if R else None
    P, p0 = piece_ptr.size - 1, 0
    while p0 < P:
        p1 = p0 + 1
        while p1 < P and (piece_ptr[p1 + 1] - piece_ptr[p0]) * slab <= budget_bytes:
            p1 += 1
        idx_h = keep[piece_ptr[p0]:piece_ptr[p1]]
        idx = torch.as_tensor(idx_h).to(dev)
        local = piece_ptr[p0:p1 + 1] - piece_ptr[p0]
        T = idx_h.size
        partner = np.arange(1, T + 1, dtype=np.int32)
        partner[local[1:] - 1] = -1
        sub = Ensemble(k[idx], edges[idx], sigma[idx], None, None, ens.thin, None)
        d2 = cross_distance(sub, rows[idx], partner, z0, z1, measure=measure, squared=True)
        res = track(d2, g[idx_h], local, n_used[idx], score=None if score is None else score[idx], marginals=marginals)
        st = res["state"].long()
        state[idx] = res["state"]
        t = torch.arange(T, device=dev)
        nxt = torch.as_tensor(np.where(partner >= 0, partner, 0).astype(np.int64)).to(dev)
        chosen = d2[t, st, st[nxt]]
        step_distance[idx] = torch.where(torch.as_tensor(partner >= 0).to(dev), torch.sqrt(chosen), torch.full_like(chosen, nan))
        own = torch.as_tensor(owner[p0:p1]).to(dev)
        log_score.index_add_(0, own, res["log_score"])
        if marginals:
            weight[idx] = res["marginal"]
            log_partition.index_add_(0, own, res["log_partition"])
        if R:
            sc = None if score is None else score[idx]
            ds = draw(d2, g[idx_h], local, n_used[idx], R, seed=seed, score=sc, row_key=idx_h)["draw_state"]
            draw_state[:, idx] = ds
            dl = ds.long()
            cost = torch.as_tensor(g[idx_h]).to(dev)[None, :] * d2[t[None, :], dl, dl[:, nxt]]
            terms = -torch.where(torch.as_tensor(partner >= 0).to(dev)[None, :], cost, torch.zeros((), **f64))
            if sc is not None:
                terms = torch.gather(sc[None, :, :].expand(R, T, n), 2, dl[:, :, None])[:, :, 0] + terms
            runs = _run_sums(terms, local)
            for q in range(p1 - p0):                                         # run after run: a cut sequence sums its runs in their order
                draw_log_score[:, int(owner[p0 + q])] += runs[:, q]
            del ds, dl, cost, terms
        del d2, res
        p0 = p1
    has = state >= 0
    nanv = torch.full((), nan, **f64)
    out = _chosen_models(k, edges, sigma, rows, n_used, state)
    out.update(step_distance=step_distance, log_score=log_score)
    if marginals:
        w = torch.where(has[:, None], weight, torch.zeros((), **f64))
        out["weight"] = weight
        out["chosen_weight"] = torch.where(has, torch.gather(w, 1, state.long().clamp(min=0)[:, None])[:, 0], nanv) if S else torch.zeros(0, **f64)
        out["n_effective"] = torch.where(has, 1.0 / (w * w).sum(dim=1), nanv)
        out["log_partition"] = log_partition
    if R:
        dhas = draw_state >= 0
        dslot = torch.gather(rows.long()[None, :, :].expand(R, S, n), 2, draw_state.long().clamp(min=0)[:, :, None])[:, :, 0].clamp(min=0)
        out.update(draw_state=draw_state, draw_slot=torch.where(dhas, dslot, torch.full_like(dslot, -1)).to(torch.int32), draw_log_score=draw_log_score)
    if boreholes is not None:
        out.update(_bh.section_outputs(b_att, b_score, b_part, b_skipped, out.get("weight"), n_used))
    if products is not None:
        out.update(lateral_products(ens, out, **products))
    if bodies is not None:
        out.update(_body_products(ens, out["draw_slot"], x, y, p, dict(bodies, group_ptr=p)))
    return out


def _chosen_models(k, edges, sigma, rows, n_used, state):
    """What ``sections`` and ``spatial`` return of the chosen models: ``state``, ``slot`` (-1: none), ``rows``, ``n_used``, ``section_k``
    (0: none) and ``section_edges`` / ``section_sigma`` (bit copies of the chosen slots; NaN: none)."""
    S, dev = k.shape[0], k.device
    has = state >= 0
    at = torch.arange(S, device=dev)
    slot = torch.gather(rows.long(), 1, state.long().clamp(min=0)[:, None])[:, 0].clamp(min=0) if S else torch.zeros(0, dtype=torch.int64, device=dev)
    nanv = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    return dict(state=state, slot=torch.where(has, slot, torch.full_like(slot, -1)).to(torch.int32), rows=rows, n_used=n_used,
                section_k=torch.where(has, k[at, slot], torch.zeros_like(k[at, slot])),
                section_edges=torch.where(has[:, None], edges[at, slot], nanv), section_sigma=torch.where(has[:, None], sigma[at, slot], nanv))


PRODUCT_KEYS = ("depth_edges", "percentiles", "thresholds")


def check_products(products):
    """``products`` of ``sections`` as the keywords of ``lateral_products``: a dictionary with ``depth_edges`` [n_depth + 1] and, optionally,
    ``percentiles`` (default 5, 50, 95) and ``thresholds`` (log10 S/m; default none).  Refuses before any device work."""
    from .ensembles import centres, check_percentiles, check_thresholds
    if not isinstance(products, dict) or "depth_edges" not in products or not set(products) <= set(PRODUCT_KEYS):
        raise ValueError("sections: products is a dictionary with depth_edges and optionally percentiles and thresholds")
    centres(products["depth_edges"])
    return dict(depth_edges=np.asarray(products["depth_edges"], dtype=np.float64), percentiles=check_percentiles(products.get("percentiles", (5, 50, 95))),
                thresholds=tuple(float(t) for t in check_thresholds(products.get("thresholds", ()))))


def lateral_products(ens, s, depth_edges, percentiles=(5, 50, 95), thresholds=()):
    """The laterally informed posterior of every sounding on a depth axis: the kept models of ``ens`` re-weighted by the smoothed
    marginals of a result ``s`` of ``sections`` (its ``rows``, ``n_used`` and ``weight``: ``marginals=True``), through
    ``ensembles.weighted`` (gbp_ensemble_weighted).  Returns on the device ``lateral_mean``, ``lateral_sd``,
    ``lateral_percentile_<p>`` f64 [S, n_depth] of log10 conductivity at the centres of ``depth_edges`` [n_depth + 1] and
    ``lateral_exceedance`` f64 [S, n_t, n_depth], the probability of log10 conductivity >= each of ``thresholds``; a sounding without
    models gives rows of NaN.  The percentiles are weighted type-1 quantiles (a value one of the models holds): where a sounding's
    posterior has two families, the median takes the value of the family its neighbours support -- a section with a credible band,
    where the Viterbi path has no spread and ``draws`` would have to be rastered and counted."""
    from .ensembles import weighted
    missing = [name for name in ("rows", "n_used", "weight") if name not in s]
    if missing:
        raise ValueError("sections.lateral_products: the result holds no %s (sections(..., marginals=True) gives the weights)" % ", ".join(missing))
    w = weighted(ens, depth_edges, s["rows"], s["weight"], n_used=s["n_used"], percentiles=percentiles, thresholds=thresholds)
    return {"lateral_" + name: v for name, v in w.items() if name not in ("weight_total", "n_effective")}


def draw_models(ens, draw_slot, depth_edges=None, log10=True):
    """The models of joint realisations: ``draw_slot`` int32 [R, S] (``sections(..., draws=R)``; -1: none) into the ensemble ``ens``.
    Returns on the device ``k`` int32 [R, S] (0: none), ``edges`` / ``sigma`` f64 [R, S, K] (bit copies of the drawn slots; NaN: none),
    and with ``depth_edges`` [n_depth + 1] ``raster`` f64 [R, S, n_depth]: ``ensembles.realisations`` (its ``log10``) of the gathered
    models -- the section of every realisation on a depth axis."""
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    are_tensors((k, edges, sigma, draw_slot), "sections", "draw_models", "gbp_ensemble_raster")
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or tuple(edges.shape[:2]) != tuple(k.shape):
        raise ValueError("ensemble: k [S, n_slots], edges and sigma [S, n_slots, K]")
    if draw_slot.ndim != 2 or draw_slot.shape[1] != k.shape[0] or draw_slot.shape[0] < 1 or draw_slot.dtype != torch.int32:
        raise ValueError("draw_models: draw_slot is int32 [R, S] with R >= 1")
    on_device((k, edges, sigma, draw_slot), "sections", "draw_models", "gbp_ensemble_raster")
    if bool(((draw_slot < -1) | (draw_slot >= k.shape[1])).any()):
        raise ValueError("draw_models: every slot must lie in -1 .. n_slots - 1")
    S, dev = k.shape[0], k.device
    has = draw_slot >= 0
    slot = draw_slot.long().clamp(min=0)
    at = torch.arange(S, device=dev)[None, :]
    nanv = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    out = dict(k=torch.where(has, k[at, slot], torch.zeros((), dtype=k.dtype, device=dev)),
               edges=torch.where(has[:, :, None], edges[at, slot], nanv), sigma=torch.where(has[:, :, None], sigma[at, slot], nanv))
    if depth_edges is not None:
        parts = []
        for r0 in range(0, draw_slot.shape[0], 4096):                         # the raster takes up to 4096 models per sounding
            sl = slice(r0, r0 + 4096)
            sub = Ensemble(out["k"][sl].t().contiguous(), out["edges"][sl].permute(1, 0, 2).contiguous(), out["sigma"][sl].permute(1, 0, 2).contiguous(),
                           None, None, ens.thin, None)
            parts.append(realisations(sub, depth_edges, log10=log10).permute(1, 0, 2))
        out["raster"] = torch.cat(parts).contiguous()
    return out


def section_widths(x, y, ptr=None):
    """float64 [S] (numpy): the along-line width a sounding stands for -- half the distance to each neighbour in its sequence of
    ``ptr`` (None: one sequence); a sequence's end has one neighbour and takes the whole distance to it (half of it on either side);
    a sequence of one sounding has no width."""
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != y.size:
        raise ValueError("sections: x and y must have one entry per sounding")
    S = x.size
    p = _default_ptr(ptr, S)
    gap = np.zeros(S + 1)                                                      # gap[s]: the distance from s - 1 to s within a sequence
    if S > 1:
        gap[1:-1] = np.hypot(np.diff(x), np.diff(y))
    gap[p] = 0.0
    before, after = gap[:-1], gap[1:]
    first, last = np.zeros(S, dtype=bool), np.zeros(S, dtype=bool)
    if S:
        first[p[:-1]], last[p[1:] - 1] = True, True
    return np.where(first, after, np.where(last, before, 0.5 * before + 0.5 * after))


def exceedance_area(k, edges, sigma, x, y, ptr, threshold, z0, z1, above=True):
    """f64 [R, L] on the models' device, m^2: per realisation and sequence of ``ptr`` [L + 1] (None: one sequence) the area of the
    section within the depth window [z0, z1] whose conductivity is >= ``threshold`` (S/m; ``above=False``: < threshold) -- the sum over
    the soundings of ``section_widths`` times the thickness of the qualifying layers clipped to the window.  ``k`` [R, S], ``edges`` /
    ``sigma`` [R, S, K]: what ``draw_models`` returns (a sounding without a model adds nothing); ``x``, ``y`` [S] (host; m).  A quantity
    of the line: it has a posterior only over joint realisations.  Plain torch; ``exceedance_area_reference`` states the rule."""
    if not (torch.is_tensor(k) and torch.is_tensor(edges) and torch.is_tensor(sigma)):
        raise ValueError("exceedance_area: k, edges and sigma are torch tensors (draw_models)")
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or tuple(edges.shape[:2]) != tuple(k.shape):
        raise ValueError("exceedance_area: k [R, S], edges and sigma [R, S, K]")
    threshold = _check_number(threshold, "threshold", positive=False)
    z0, z1 = _check_number(z0, "z0", positive=False), _check_number(z1, "z1", positive=False)
    if not 0.0 <= z0 < z1:
        raise ValueError("exceedance_area: the window needs 0 <= z0 < z1")
    R, S, K = edges.shape
    if np.size(x) != S or np.size(y) != S:
        raise ValueError("exceedance_area: x and y must hold one entry per sounding (%d)" % S)
    p = _default_ptr(ptr, S)
    width = torch.as_tensor(section_widths(x, y, p)).to(edges.device)
    layer = torch.arange(K, device=edges.device)[None, None, :]
    kk = k.long()[:, :, None]
    inf = torch.full((), float("inf"), dtype=torch.float64, device=edges.device)
    zero = torch.zeros((), dtype=torch.float64, device=edges.device)
    top = torch.cat([torch.zeros((R, S, 1), dtype=torch.float64, device=edges.device), edges[:, :, :-1]], dim=2)
    bottom = torch.where(layer < kk - 1, edges, inf)
    counts = (layer < kk) & ((sigma >= threshold) if above else (sigma < threshold))
    thick = torch.where(counts, (bottom.clamp(max=z1) - top.clamp(min=z0)).clamp(min=0.0), zero).sum(dim=2)
    return _run_sums(width[None, :] * thick, p)


# ---- connected bodies of the realisations ----------------------------------------------------------------------------

BODY_KEYS = ("depth_edges", "lo", "hi", "log10", "surface", "elevation_edges", "a", "min_cells")


def check_bodies(bodies, what):
    """``bodies`` of ``sections`` / ``spatial`` as keywords of ``draw_bodies``: a dictionary with ``depth_edges`` and optionally ``lo``,
    ``hi``, ``log10``, ``surface``, ``elevation_edges``, ``a`` and ``min_cells``.  Refuses before any device work."""
    from .ensembles import centres
    if not isinstance(bodies, dict) or "depth_edges" not in bodies or not set(bodies) <= set(BODY_KEYS):
        raise ValueError("%s: bodies is a dictionary with depth_edges and optionally %s" % (what, ", ".join(BODY_KEYS[1:])))
    centres(bodies["depth_edges"])
    if "lo" in bodies or "hi" in bodies:
        from .bodies import _check_bounds
        _check_bounds(bodies.get("lo", -np.inf), bodies.get("hi", np.inf), what + ": bodies")
    return dict(bodies, depth_edges=np.asarray(bodies["depth_edges"], dtype=np.float64))


def line_edges(ptr):
    """(eu, ev) int64: the consecutive pairs inside every sequence of ``ptr`` [L + 1] -- the graph of a survey whose lines stand alone."""
    p = np.asarray(ptr, dtype=np.int64)
    S = int(p[-1]) if p.size else 0
    last = np.zeros(S, dtype=bool)
    last[p[1:][p[1:] > p[:-1]] - 1] = True
    eu = np.flatnonzero(~last).astype(np.int64)
    return eu, eu + 1


def draw_bodies(ens, draw_slot, depth_edges, x, y, ptr, lo=-np.inf, hi=np.inf, log10=True, eu=None, ev=None, surface=None, elevation_edges=None,
                a=None, group_ptr=None, **summary_kw):
    """The connected bodies of joint realisations: ``draw_models(ens, draw_slot, depth_edges, log10)`` rasters the
    drawn models [R, S, n_depth]; with ``surface`` [S] (the soundings' elevation) ``elevation.resample`` takes the raster onto ONE
    elevation axis ``elevation_edges`` (default ``elevation.regular_axis`` at the thinnest depth cell's width; NaN, never a member,
    outside a sounding's mesh), so that lateral adjacency is horizontal; ``bodies.label`` labels the bodies of the cells with lo <=
    value <= hi (log10 S/m with ``log10``) over the edges ``eu`` / ``ev`` (default: the consecutive pairs inside ``ptr``: every line
    alone; ``edge_u`` / ``edge_v`` of ``spatial`` join the lines) with ``a`` [S] (default ``section_widths``: the measure is an area
    in m^2; ``bodies.sounding_areas`` makes it a volume) and the cells' thickness; ``bodies.summary`` (``summary_kw``) sums them up.
    Returns what ``label`` and ``summary`` return, plus ``a`` and ``t`` (numpy)."""
    from . import bodies as body_labels, elevation
    e = elevation.check_depth_edges(depth_edges)
    S = ens.k.shape[0]
    p = _default_ptr(ptr, S)
    if (eu is None) != (ev is None):
        raise ValueError("sections.draw_bodies: eu and ev are given together or not at all")
    if eu is None:
        eu, ev = line_edges(p)
    a = section_widths(x, y, p) if a is None else np.asarray(host(a), dtype=np.float64).reshape(-1)
    if surface is not None:
        axis = elevation.regular_axis(surface, e, float(np.diff(e).min())) if elevation_edges is None else elevation.check_axis(edges=elevation_edges)[1]
    raster = draw_models(ens, draw_slot, depth_edges=e, log10=log10)["raster"]
    if surface is None:
        t = np.diff(e)
    else:
        raster = elevation.resample(raster.permute(1, 0, 2).contiguous(), surface, e, edges=axis).permute(1, 0, 2).contiguous()
        t = np.diff(axis)
    lab = body_labels.label(raster, lo, hi, eu, ev, group_ptr=group_ptr, a=a, t=t)
    lab.update(body_labels.summary(lab, **summary_kw))
    lab.update(a=a, t=t)
    return lab


def _body_products(ens, draw_slot, x, y, ptr, kw):
    """``body_count``, ``body_largest_measure``, ``body_member_measure`` [R, G] and ``body_largest_share`` [S, C] of ``draw_bodies``."""
    from .bodies import _cell_groups
    b = draw_bodies(ens, draw_slot, x=x, y=y, ptr=ptr, **kw)
    R, S, C = b["label"].shape
    gid, _ = _cell_groups(b)
    flat = b["label"].reshape(R, S * C).long()
    own = torch.gather(b["largest_root"], 1, gid[None, :].expand(R, S * C)) if S * C else flat
    share = ((flat >= 0) & (flat == own)).to(torch.float64).mean(dim=0).reshape(S, C)
    return dict(body_count=b["n_bodies"], body_largest_measure=b["largest_measure"], body_member_measure=b["member_measure"], body_largest_share=share)


# ---- across lines: belief propagation on the survey graph -----------------------------------------------------------

MAX_GRAPH_STATES = 256
MAX_SWEEPS = 65536
SPATIAL_SUFFIX = ".spatial.npz"


def _check_damping(damping, what):
    if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) or not 0.0 <= damping < 1.0:
        raise ValueError("%s: damping must be a number in [0, 1)" % what)
    return float(damping)


def _check_graph(eu, ev, g, d2, n_used, score, sweeps, damping, what):
    """The host checks ``propagate`` and its reference share; returns eu, ev (numpy int64 [E]), n_used (numpy int64 [S]), sweeps and
    damping."""
    if d2.ndim != 3 or d2.shape[1] != d2.shape[2] or not 1 <= d2.shape[1] <= MAX_GRAPH_STATES:
        raise ValueError("%s: d2 [E, n, n] with 1 <= n <= %d" % (what, MAX_GRAPH_STATES))
    E, n = d2.shape[0], d2.shape[1]
    nu = host(n_used).reshape(-1)
    S = nu.size
    if nu.dtype.kind not in "iu":
        raise ValueError("%s: n_used must hold one integer per sounding" % what)
    if np.any(nu < 1) or np.any(nu > n):
        raise ValueError("%s: n_used must lie in 1 .. n (soundings without models are left out of the graph)" % what)
    eu, ev = host(eu).reshape(-1), host(ev).reshape(-1)
    if eu.size != E or ev.size != E or eu.dtype.kind not in "iu" or ev.dtype.kind not in "iu":
        raise ValueError("%s: eu and ev must hold one integer per edge (%d)" % (what, E))
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    if np.any(eu < 0) or np.any(ev >= S) or np.any(eu >= ev):
        raise ValueError("%s: every edge needs 0 <= eu < ev < the number of soundings (%d)" % (what, S))
    if np.any(np.diff(eu * S + ev) <= 0):
        raise ValueError("%s: the edges must be sorted by (eu, ev) and hold no duplicates" % what)
    if host(g).size != E:
        raise ValueError("%s: g must hold one entry per edge" % what)
    if score is not None and tuple(score.shape) != (S, n):
        raise ValueError("%s: score must be [S, n]" % what)
    return eu, ev, nu.astype(np.int64), check_int(sweeps, 1, MAX_SWEEPS, "%s: sweeps" % what), _check_damping(damping, what)


def incoming(eu, ev, n_soundings):
    """The CSR of every sounding's incoming directed edges (numpy int32): ``in_ptr`` [S + 1] and ``in_edge`` [2 E], sorted by the
    sounding a message comes from.  Directed edge 2 e is eu[e] -> ev[e], 2 e + 1 is ev[e] -> eu[e]."""
    eu, ev = np.asarray(eu, dtype=np.int64).reshape(-1), np.asarray(ev, dtype=np.int64).reshape(-1)
    src, dst = np.empty(2 * eu.size, dtype=np.int64), np.empty(2 * eu.size, dtype=np.int64)
    src[0::2], dst[0::2], src[1::2], dst[1::2] = eu, ev, ev, eu
    in_edge = np.lexsort((src, dst)).astype(np.int32)
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=int(n_soundings)))]).astype(np.int32)
    return in_ptr, in_edge


def _nan_max(r, d):
    """max that keeps a NaN once it has one."""
    return d if (d > r or d != d) else r


def propagate_reference(eu, ev, g, d2, n_used, score=None, sweeps=32, damping=0.0, dtype=np.float64, keep_messages=False):
    """The rule of ``propagate`` in numpy, evaluated in ``dtype`` (fp64: what the device is held to; np.longdouble: the yardstick of the
    rule's own rounding): synchronous sum-product message passing on the graph of S = len(n_used) soundings with the undirected edges
    ``eu[e]`` < ``ev[e]`` (sorted by (eu, ev), no duplicates), ``g`` [E] and ``d2`` [E, n, n], entry [e, i, j] between state i of
    eu[e] and state j of ev[e]; only the prefixes i < m_u, j < m_v are read (m_s = n_used[s] in 1 .. n).

    w_s = exp(score[s]) (None: ones); K_e = exp(-(g[e] * d2[e])), one multiply and one exp per entry.  Directed edge 2 e is u -> v
    and uses K_e, 2 e + 1 is v -> u and uses its transpose; the message mu[d] has m_dst entries and starts at 1 / m_dst.  One sweep
    computes every message from the last sweep's.  For a -> b: h[i] = w_a[i] times mu[c -> a][i] over the neighbours c != b of a,
    ascending c; u[j] = sum_i h[i] K[i, j], i ascending, u = u + h[i] * K[i]; tot = sum_j u[j], j ascending; mu' = u / tot; with
    ``damping`` = lam != 0 mu' = (1 - lam) mu' + lam mu_old (lam = 0 skips the blend).  ``residual[t]`` is the largest |mu' - mu_old|
    over the messages of sweep t (NaN if one of them is; 0.0 without edges).  After the last sweep belief_s = w_s times all incoming
    messages (ascending neighbour), divided by its sum (i ascending), 0.0 for the states >= m_s; ``state[s]`` is its first maximum.
    A sounding without edges gets its normalised w.  A zero tot gives NaN, as a zero scale does in ``track_reference``.

    Exact on a tree once the sweeps reach its diameter (the residual is 0.0 from then on: every message has its final bits); on a
    graph with loops a documented approximation: the output is a *belief*, not a marginal.

    Returns ``belief`` [S, n] (``dtype``), ``state`` int32 [S] and ``residual`` [sweeps]; with ``keep_messages`` also ``message``
    [2 E, n], the messages after the last sweep (0.0 beyond m_dst), and ``node_weight`` [S, n], w (0.0 beyond m_s)."""
    ft = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    eu, ev, nu, sweeps, damping = _check_graph(eu, ev, g, d2, n_used, score, sweeps, damping, "sections.propagate_reference")
    E, n, S = d2.shape[0], d2.shape[1], nu.size
    g = np.asarray(g, dtype=np.float64).reshape(-1).astype(ft)
    w = [np.exp((np.zeros(nu[s]) if score is None else score[s, :nu[s]]).astype(ft)) for s in range(S)]
    K = [np.exp(-(g[e] * d2[e, :nu[eu[e]], :nu[ev[e]]].astype(ft))) for e in range(E)]
    in_ptr, in_edge = incoming(eu, ev, S)
    src = np.empty(2 * E, dtype=np.int64)
    src[0::2], src[1::2] = eu, ev
    dst = np.empty(2 * E, dtype=np.int64)
    dst[0::2], dst[1::2] = ev, eu
    inc = [in_edge[in_ptr[s]:in_ptr[s + 1]] for s in range(S)]
    msg = [np.full(nu[dst[d]], ft(1) / ft(nu[dst[d]]), dtype=ft) for d in range(2 * E)]
    lam = ft(damping)
    residual = np.zeros(sweeps, dtype=ft)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(sweeps):
            new, r = [], ft(0)
            for d in range(2 * E):
                a, b = int(src[d]), int(dst[d])
                h = w[a].copy()
                for q in inc[a]:                                             # ascending neighbour
                    if src[q] != b:
                        h = h * msg[q]
                Kd = K[d // 2] if d % 2 == 0 else K[d // 2].T
                u = np.zeros(nu[b], dtype=ft)
                for i in range(nu[a]):                                       # i ascending
                    u = u + h[i] * Kd[i]
                tot = ft(0)
                for j in range(nu[b]):                                       # j ascending
                    tot = tot + u[j]
                m = u / tot
                if damping != 0.0:
                    m = (ft(1) - lam) * m + lam * msg[d]
                r = _nan_max(r, np.abs(m - msg[d]).max())
                new.append(m)
            msg = new
            residual[t] = r
        belief, state = np.zeros((S, n), dtype=ft), np.zeros(S, dtype=np.int32)
        for s in range(S):
            h = w[s].copy()
            for q in inc[s]:
                h = h * msg[q]
            tot = ft(0)
            for i in range(nu[s]):
                tot = tot + h[i]
            belief[s, :nu[s]] = h / tot
            state[s] = first_max(belief[s, :nu[s]])
    out = dict(belief=belief, state=state, residual=residual)
    if keep_messages:
        message, node_weight = np.zeros((2 * E, n), dtype=ft), np.zeros((S, n), dtype=ft)
        for d in range(2 * E):
            message[d, :nu[dst[d]]] = msg[d]
        for s in range(S):
            node_weight[s, :nu[s]] = w[s]
        out.update(message=message, node_weight=node_weight)
    return out


def neighbours(x, y, ptr=None, n_used=None, *, max_distance, tau=0.1, length=100.0, min_distance=1.0):
    """The survey graph (host, numpy): ``eu``, ``ev`` int32 [E] with eu < ev, sorted by (eu, ev) without duplicates, ``g`` float64
    [E] and ``dist`` float64 [E] (m) for soundings at ``x``, ``y`` [S] in the sequences of ``ptr`` [L + 1] (None: one sequence).
    Along a line the edges are exactly the pairs ``partners(ptr, n_used)`` connects.  Across lines every sounding with models
    (``n_used`` > 0; None: all) is joined to the nearest sounding with models of every *other* sequence -- a tie goes to the lowest
    index -- if that distance is <= ``max_distance``; the union is undirected.  g = length / (2 tau^2 max(dist, min_distance)): the
    convention of ``steps``, applied to the edge's horizontal distance.  ``max_distance`` is required: about 1.5 line spacings is the
    natural value, and it is not guessed.  Lines are taken pair by pair, a pair whose bounding boxes lie further apart than
    ``max_distance`` is skipped, and the distances of one pair are held at a time: memory is O(longest line^2)."""
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != y.size:
        raise ValueError("sections.neighbours: x and y must have one entry per sounding")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("sections.neighbours: x and y must be finite")
    S = x.size
    max_distance = _check_number(max_distance, "max_distance")
    tau, length, min_distance = _check_number(tau, "tau"), _check_number(length, "length"), _check_number(min_distance, "min_distance")
    p = _default_ptr(ptr, S)
    nu = np.ones(S, dtype=np.int64) if n_used is None else host(n_used).reshape(-1)
    if nu.size != S or nu.dtype.kind not in "iu":
        raise ValueError("sections.neighbours: n_used must hold one integer per sounding")
    partner = partners(p, nu).astype(np.int64)
    has = np.flatnonzero(partner >= 0)
    keys = [has * S + partner[has]]
    members = [a + np.flatnonzero(nu[a:b] > 0) for a, b in zip(p[:-1], p[1:])]
    boxes = [(x[m].min(), x[m].max(), y[m].min(), y[m].max()) if m.size else None for m in members]
    for la in range(len(members)):
        for lb in range(la + 1, len(members)):
            A, B = members[la], members[lb]
            if not A.size or not B.size:
                continue
            ba, bb = boxes[la], boxes[lb]
            gap_x, gap_y = max(ba[0] - bb[1], bb[0] - ba[1], 0.0), max(ba[2] - bb[3], bb[2] - ba[3], 0.0)
            if np.hypot(gap_x, gap_y) > max_distance:
                continue
            D = np.hypot(x[A][:, None] - x[B][None, :], y[A][:, None] - y[B][None, :])
            ja, ib = np.argmin(D, axis=1), np.argmin(D, axis=0)              # the first minimum: the lowest index
            near = D[np.arange(A.size), ja] <= max_distance
            keys.append(np.minimum(A[near], B[ja[near]]) * S + np.maximum(A[near], B[ja[near]]))
            near = D[ib, np.arange(B.size)] <= max_distance
            keys.append(np.minimum(A[ib[near]], B[near]) * S + np.maximum(A[ib[near]], B[near]))
    key = np.unique(np.concatenate(keys)) if S else np.zeros(0, dtype=np.int64)
    eu, ev = (key // S, key % S) if S else (key, key)
    dist = np.hypot(x[ev] - x[eu], y[ev] - y[eu])
    return eu.astype(np.int32), ev.astype(np.int32), length / (2.0 * tau * tau * np.maximum(dist, min_distance)), dist


def edge_distance(ens, rows, eu, ev, z0, z1, measure="linear"):
    """D^2 f64 [E, n, n] on the device for the edges ``eu`` < ``ev`` (host; sorted by (eu, ev)): entry [e, i, j] is the squared
    distance of ``cross_distance`` between model ``rows[eu[e], i]`` and model ``rows[ev[e], j]``.  No kernel of its own: pass p calls
    ``cross_distance`` with every sounding paired with its p-th higher-indexed neighbour and copies the slabs out, so every entry has
    that kernel's bits; the passes are as many as the largest number of higher-indexed neighbours of a sounding."""
    are_tensors((ens.k, ens.edges, ens.sigma, rows), "sections", "edge_distance", "gbp_ensemble_cross_distance")
    S = ens.k.shape[0]
    eu, ev = host(eu).reshape(-1), host(ev).reshape(-1)
    if eu.size != ev.size or eu.dtype.kind not in "iu" or ev.dtype.kind not in "iu":
        raise ValueError("sections.edge_distance: eu and ev must hold one integer per edge")
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    if np.any(eu < 0) or np.any(ev >= S) or np.any(eu >= ev) or np.any(np.diff(eu * S + ev) <= 0):
        raise ValueError("sections.edge_distance: the edges need 0 <= eu < ev < S, sorted by (eu, ev) without duplicates")
    E = eu.size
    if rows.ndim != 2:
        raise ValueError("sections.edge_distance: rows [S, n]")
    n = rows.shape[1]
    first = np.searchsorted(eu, eu, side="left")                              # the first edge of every edge's lower sounding
    rank = np.arange(E) - first
    out = None
    for p in range(int(rank.max(initial=-1)) + 1):
        at = np.flatnonzero(rank == p)
        partner = np.full(S, -1, dtype=np.int32)
        partner[eu[at]] = ev[at]
        d = cross_distance(ens, rows, partner, z0, z1, measure=measure, squared=True)
        if out is None:
            out = torch.empty((E, n, n), dtype=torch.float64, device=d.device)
        out[torch.as_tensor(at).to(d.device)] = d[torch.as_tensor(eu[at]).to(d.device)]
        del d
    if out is None:
        check_window(z0, z1, measure)
        on_device((ens.k, rows), "sections", "edge_distance", "gbp_ensemble_cross_distance")
        out = torch.empty((0, n, n), dtype=torch.float64, device=rows.device)
    return out


def propagate(d2, g, eu, ev, n_used, n_soundings, score=None, sweeps=32, damping=0.0, keep_kernel=False, keep_messages=False):
    """Beliefs of the graph of ``propagate_reference`` on the device (gbp_section_propagate: csrc/gbp_section_graph.h): ``d2`` f64
    [E, n, n] on the device (``edge_distance``), n <= 256; ``g`` [E], ``eu`` < ``ev`` [E] (host or device; sorted by (eu, ev), no
    duplicates), ``n_used`` [S] in 1 .. n with S = ``n_soundings``, ``score`` f64 [S, n] on the device or None: zeros; ``sweeps`` >= 1
    synchronous sweeps with ``damping`` in [0, 1).  Returns on the device ``belief`` f64 [S, n], ``state`` int32 [S] (the first maximum
    of the belief) and ``residual`` f64 [sweeps] (the largest change of a message per sweep: 0.0 once a tree has converged).  d2 is
    left as it is; K = exp(-(g d2)) takes a second buffer of its size.  The CSR of incoming edges is made once on the host.
    ``keep_kernel`` adds that K buffer as ``kernel`` f64 [E, n, n] (valid on the prefixes i < m_u, j < m_v): what ``graph_draw`` takes
    as ``kernel=``; ``keep_messages`` adds ``message`` f64 [2 E, n], the messages after the last sweep, and ``node_weight`` f64 [S, n],
    w = exp(score): what ``graph_terms`` takes."""
    entry = "gbp_section_propagate"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "propagate", entry)
    S = check_int(n_soundings, 0, 2 ** 31 - 1, "sections.propagate: n_soundings")
    if np.size(host(n_used)) != S:
        raise ValueError("sections.propagate: n_used must hold one integer per sounding (%d)" % S)
    eu, ev, nu, sweeps, damping = _check_graph(eu, ev, g, d2, n_used, score, sweeps, damping, "sections.propagate")
    if d2.dtype != torch.float64 or (score is not None and score.dtype != torch.float64):
        raise TypeError("sections.propagate: d2 and score are float64")
    on_device((d2,) + (() if score is None else (score,)), "sections", "propagate", entry)
    dev = d2.device
    E, n = d2.shape[0], d2.shape[1]
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(belief=torch.empty((S, n), **f64), state=torch.empty(S, **i32), residual=torch.zeros(sweeps, **f64))
    if S == 0:
        if keep_kernel:
            out["kernel"] = torch.empty_like(d2)
        if keep_messages:
            out.update(message=torch.empty((2 * E, n), **f64), node_weight=torch.empty((0, n), **f64))
        return out
    in_ptr, in_edge = incoming(eu, ev, S)
    d2 = d2.contiguous()
    score = torch.zeros((S, n), **f64) if score is None else score.contiguous()
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev) if not torch.is_tensor(g) else g.to(dev, torch.float64).reshape(-1).contiguous()
    t_eu, t_ev, t_nu = (torch.as_tensor(a.astype(np.int32)).to(dev) for a in (eu, ev, nu))
    t_ptr, t_edge = torch.as_tensor(in_ptr).to(dev), torch.as_tensor(in_edge).to(dev)
    K, w = torch.empty_like(d2), torch.empty((S, n), **f64)
    mu, resid = torch.empty((2, 2 * E, n), **f64), torch.empty((sweeps, 2 * E), **f64)
    _lib.call(entry, dev, S, E, n, t_eu, t_ev, t_nu, score, t_g, d2, t_ptr, t_edge, sweeps, damping, K, w, mu, resid, out["belief"], out["state"],
              out["residual"])
    if keep_kernel:
        out["kernel"] = K
    if keep_messages:
        out.update(message=mu[sweeps & 1], node_weight=w)
    return out


# ---- across lines: the Bethe evidence of the coupling ------------------------------------------------------------

def graph_rank(eu, ev, n_soundings):
    """The number of soundings minus the number of connected components of the graph: the degrees of freedom of the Gaussian step
    field, whose normaliser grows as c^(rank / 2).  A loop adds an edge and no rank."""
    eu, ev, S = _check_edges(eu, ev, n_soundings, "sections.graph_rank")
    root = list(range(S))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    rank = 0
    for a, b in zip(eu.tolist(), ev.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            root[ra] = rb
            rank += 1
    return rank


def graph_terms_reference(eu, ev, g, d2, n_used, node_weight, message, dtype=np.float64):
    """The rule of gbp_section_graph_evidence in numpy, evaluated in ``dtype``: from the messages [2 E, n] and weights [S, n] that
    ``propagate_reference(..., keep_messages=True)`` returns, per edge e = {u, v} h_u = w_u times the messages into u but v's, h_v
    likewise (ascending neighbour), K = exp(-(g[e] * d2[e])), ``edge_log_z`` [E] = ln sum_ij h_u[i] K_ij h_v[j] and ``edge_energy``
    [E] = g[e] sum_ij h_u[i] K_ij d2_ij h_v[j] / that sum; per sounding ``node_log_z`` [S] = ln sum_i w_s[i] times all its incoming
    messages.  Prefixes only; the sums are numpy's: their order is not part of the rule."""
    ft = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=np.float64)
    eu, ev, nu, _, _ = _check_graph(eu, ev, g, d2, n_used, None, 1, 0.0, "sections.graph_terms_reference")
    E, n, S = d2.shape[0], d2.shape[1], nu.size
    node_weight, message = np.asarray(node_weight), np.asarray(message)
    if node_weight.shape != (S, n) or message.shape != (2 * E, n):
        raise ValueError("sections.graph_terms_reference: node_weight [S, n] and message [2 E, n]")
    g = np.asarray(host(g), dtype=np.float64).reshape(-1).astype(ft)
    in_ptr, in_edge = incoming(eu, ev, S)
    src = np.empty(2 * E, dtype=np.int64)
    src[0::2], src[1::2] = eu, ev

    def h(a, but):
        out = node_weight[a, :nu[a]].astype(ft)
        for q in in_edge[in_ptr[a]:in_ptr[a + 1]]:                            # ascending neighbour
            if src[q] != but:
                out = out * message[q, :nu[a]].astype(ft)
        return out

    node, edge, energy = np.zeros(S, dtype=ft), np.zeros(E, dtype=ft), np.zeros(E, dtype=ft)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(S):
            node[s] = np.log(h(s, -1).sum())
        for e in range(E):
            u, v = int(eu[e]), int(ev[e])
            d = d2[e, :nu[u], :nu[v]].astype(ft)
            p = h(u, v)[:, None] * np.exp(-(g[e] * d)) * h(v, u)[None, :]
            z = p.sum()
            edge[e], energy[e] = np.log(z), g[e] * (p * d).sum() / z
    return dict(node_log_z=node, edge_log_z=edge, edge_energy=energy)


def _bethe(terms, eu, ev, S, scale, log_w):
    """log Z_B = sum_s (1 - deg_s) node_log_z[s] + sum_e edge_log_z[e] and dlog Z_B = -sum_e edge_energy[e], summed on the host in
    index order over the S + 2 E doubles (float64 numpy); the log evidence adds rank / 2 ln c - sum_s ln sum_i w_s[i]."""
    node, edge, energy = (np.asarray(terms[name], dtype=np.float64) for name in ("node_log_z", "edge_log_z", "edge_energy"))
    deg = np.bincount(eu, minlength=S) + np.bincount(ev, minlength=S)
    log_z = dlog_z = 0.0
    for s in range(S):
        log_z += (1.0 - deg[s]) * node[s]
    for e in range(edge.size):
        log_z += edge[e]
        dlog_z -= energy[e]
    rank = graph_rank(eu, ev, S)
    return dict(log_partition=float(log_z), dlog_partition=float(dlog_z), rank=rank,
                log_evidence=float(log_z + 0.5 * rank * np.log(scale) - np.sum(log_w)))


def graph_evidence_reference(eu, ev, g, d2, n_used, score=None, scale=1.0, sweeps=32, damping=0.0, dtype=np.float64):
    """The rule of ``graph_evidence``: ``propagate_reference`` with ``g`` times ``scale`` (one multiply per edge, in float64), then
    ``graph_terms_reference`` on its messages and the sums of the Bethe evidence.  Returns what ``graph_evidence`` returns, in numpy."""
    scale = _check_ladder(0.1, 1, scale, "sections.graph_evidence_reference")[2]
    gs = np.asarray(host(g), dtype=np.float64).reshape(-1) * scale
    prop = propagate_reference(eu, ev, gs, d2, n_used, score, sweeps=sweeps, damping=damping, dtype=dtype, keep_messages=True)
    terms = graph_terms_reference(eu, ev, gs, d2, n_used, prop["node_weight"], prop["message"], dtype=dtype)
    nu = host(n_used).reshape(-1).astype(np.int64)
    out = _bethe(terms, host(eu).reshape(-1).astype(np.int64), host(ev).reshape(-1).astype(np.int64), nu.size, scale,
                 _log_weights(None if score is None else np.asarray(score, dtype=np.float64), nu))
    out.update(terms, residual=prop["residual"], belief=prop["belief"])
    return out


def graph_terms(d2, g, eu, ev, n_used, n_soundings, node_weight, message):
    """``node_log_z`` [S], ``edge_log_z`` [E] and ``edge_energy`` [E] on the device (gbp_section_graph_evidence: csrc/
    gbp_section_evidence.h k_graph_evidence; ``graph_terms_reference`` states the rule) from the ``node_weight`` and ``message`` of
    ``propagate(..., keep_messages=True)``; ``d2``, ``g``, ``eu``, ``ev``, ``n_used``, ``n_soundings`` as ``propagate`` takes them."""
    entry = "gbp_section_graph_evidence"
    are_tensors((d2, node_weight, message), "sections", "graph_terms", entry)
    S = check_int(n_soundings, 0, 2 ** 31 - 1, "sections.graph_terms: n_soundings")
    if np.size(host(n_used)) != S:
        raise ValueError("sections.graph_terms: n_used must hold one integer per sounding (%d)" % S)
    eu, ev, nu, _, _ = _check_graph(eu, ev, g, d2, n_used, None, 1, 0.0, "sections.graph_terms")
    E, n = d2.shape[0], d2.shape[1]
    if tuple(node_weight.shape) != (S, n) or tuple(message.shape) != (2 * E, n):
        raise ValueError("sections.graph_terms: node_weight [S, n] and message [2 E, n]")
    if d2.dtype != torch.float64 or node_weight.dtype != torch.float64 or message.dtype != torch.float64:
        raise TypeError("sections.graph_terms: d2, node_weight and message are float64")
    on_device((d2, node_weight, message), "sections", "graph_terms", entry)
    dev = d2.device
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(node_log_z=torch.empty(S, **f64), edge_log_z=torch.empty(E, **f64), edge_energy=torch.empty(E, **f64))
    if S == 0:
        return out
    in_ptr, in_edge = incoming(eu, ev, S)
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev)
    t_eu, t_ev, t_nu = (torch.as_tensor(a.astype(np.int32)).to(dev) for a in (eu, ev, nu))
    _lib.call(entry, dev, S, E, n, t_eu, t_ev, t_nu, node_weight.contiguous(), t_g, d2.contiguous(), torch.as_tensor(in_ptr).to(dev),
              torch.as_tensor(in_edge).to(dev), message.contiguous(), out["node_log_z"], out["edge_log_z"], out["edge_energy"])
    return out


def graph_evidence(d2, g, eu, ev, n_used, n_soundings, score=None, scale=1.0, sweeps=32, damping=0.0):
    """The Bethe evidence of the coupling on the survey graph and its derivative (``graph_evidence_reference`` states
    the rule): ``propagate`` with ``g`` times ``scale``, then ``graph_terms`` on its messages.  Arguments as ``propagate`` takes them.
    Returns floats ``log_partition`` = log Z_B = sum_s (1 - deg_s) node_log_z[s] + sum_e edge_log_z[e], ``dlog_partition`` = -sum_e
    edge_energy[e] (the derivative in lambda = ln c), ``log_evidence`` = log Z_B + rank / 2 ln scale - sum_s ln sum_i w_s[i] and
    ``rank`` (``graph_rank``), and numpy arrays ``node_log_z`` [S], ``edge_log_z`` [E], ``edge_energy`` [E] -- which edges of the
    survey are strained -- ``residual`` [sweeps] and ``belief`` [S, n].  Exact on a forest once ``sweeps`` reach its diameter; on loops
    an approximation, as the beliefs are."""
    scale = _check_ladder(0.1, 1, scale, "sections.graph_evidence")[2]
    gs = host(g).reshape(-1).astype(np.float64) * scale
    prop = propagate(d2, gs, eu, ev, n_used, n_soundings, score=score, sweeps=sweeps, damping=damping, keep_messages=True)
    terms = {name: v.cpu().numpy() for name, v in graph_terms(d2, gs, eu, ev, n_used, n_soundings, prop["node_weight"], prop["message"]).items()}
    nu = host(n_used).reshape(-1).astype(np.int64)
    out = _bethe(terms, host(eu).reshape(-1).astype(np.int64), host(ev).reshape(-1).astype(np.int64), nu.size, scale,
                 _log_weights(None if score is None else score.cpu().numpy(), nu))
    out.update(terms, residual=prop["residual"].cpu().numpy(), belief=prop["belief"].cpu().numpy())
    return out


def _graph_ladder(one, tau_max, scale, rungs):
    """The ladder result ``_fit`` takes, one ``graph_evidence`` per rung (``one(scale)``); L = 1: the graph is pooled."""
    c = scale * 2.0 ** np.arange(rungs)
    got = [one(float(v)) for v in c]
    col = lambda name: np.array([[r[name]] for r in got], dtype=np.float64)      # noqa: E731
    return dict(tau=tau_max / np.sqrt(c), scale=c, rank=np.array([got[0]["rank"]]), log_partition=col("log_partition"),
                dlog_partition=col("dlog_partition"), log_evidence=col("log_evidence"),
                residual=np.array([r["residual"][-1] for r in got], dtype=np.float64), edge_energy=np.stack([r["edge_energy"] for r in got]))


def fit_tau_graph_reference(eu, ev, g, d2, n_used, score=None, tau0=0.1, tau_max=0.8, rungs=11, sweeps=32, damping=0.0, dtype=np.float64):
    """``fit_tau_graph`` on the rules (``graph_evidence_reference``), numpy arrays throughout."""
    tau_max, rungs = _check_fit(tau_max, rungs, "sections.fit_tau_graph_reference")
    tau0 = _check_ladder(tau0, 1, 1.0, "sections.fit_tau_graph_reference")[0]
    g_max = np.asarray(host(g), dtype=np.float64).reshape(-1) * (tau0 / tau_max) ** 2
    one = lambda c: graph_evidence_reference(eu, ev, g_max, d2, n_used, score, scale=c, sweeps=sweeps, damping=damping, dtype=dtype)      # noqa: E731
    return _fit(lambda scale, T: _graph_ladder(one, tau_max, scale, T), tau_max, rungs)


def fit_tau_graph(d2, g, eu, ev, n_used, n_soundings, score=None, tau0=0.1, tau_max=0.8, rungs=11, sweeps=32, damping=0.0):
    """``fit_tau`` for the survey graph: the same ladder, bracket and refinement over ``graph_evidence``, one ``propagate`` of
    ``sweeps`` sweeps per evaluation; ``g`` (``neighbours``) at ``tau0``.  Returns what ``fit_tau`` returns -- ``log_evidence_sequence``
    is [rungs, 1], the graph is pooled -- and ``residual`` [rungs], the last sweep's residual of every rung: where the messages had not
    settled, the Bethe evidence of that rung is not at a fixed point and its derivative is not exact."""
    tau_max, rungs = _check_fit(tau_max, rungs, "sections.fit_tau_graph")
    tau0 = _check_ladder(tau0, 1, 1.0, "sections.fit_tau_graph")[0]
    g_max = host(g).reshape(-1).astype(np.float64) * (tau0 / tau_max) ** 2
    one = lambda c: graph_evidence(d2, g_max, eu, ev, n_used, n_soundings, score=score, scale=c, sweeps=sweeps, damping=damping)      # noqa: E731
    return _fit(lambda scale, T: _graph_ladder(one, tau_max, scale, T), tau_max, rungs)


# ---- across lines: joint draws by Gibbs sampling blocked by flight line ----------------------------------------------

MAX_DRAW_SWEEPS = 65535


def _line_of(ptr, S):
    """int64 [S]: the sequence of ``ptr`` every sounding lies in (empty sequences own none)."""
    return np.searchsorted(ptr, np.arange(S), side="right") - 1


def check_lines(eu, ev, ptr, S, what):
    """The sequences of a graph: ``ptr`` as int64 [L + 1] (sequences may be empty), ``step_edge`` int32 [S] (the edge of the step
    s -> s + 1; -1 at a sequence's last sounding) and ``cross`` bool [E].  An edge inside a sequence must be a step and every
    consecutive pair of a sequence must be an edge."""
    ptr = check_ptr(ptr, S, empty=True)
    line = _line_of(ptr, S)
    same = line[eu] == line[ev]
    step = same & (ev == eu + 1)
    if np.any(same & ~step):
        e = int(np.flatnonzero(same & ~step)[0])
        raise ValueError("%s: an edge inside a sequence must join consecutive soundings; edge (%d, %d) is not a step" % (what, eu[e], ev[e]))
    step_edge = np.full(S, -1, dtype=np.int32)
    step_edge[eu[step]] = np.flatnonzero(step)
    last = np.zeros(S, dtype=bool)
    last[ptr[1:][np.diff(ptr) > 0] - 1] = True
    if np.any((step_edge < 0) & ~last):
        s = int(np.flatnonzero((step_edge < 0) & ~last)[0])
        raise ValueError("%s: consecutive soundings of a sequence must be joined by an edge; the step %d -> %d is missing (cut ptr there)" % (what, s, s + 1))
    return ptr, step_edge, ~same


def line_colours(eu, ev, ptr):
    """The colour classes of the sequences of ``ptr`` [L + 1] under the edges ``eu``, ``ev`` (host): two sequences are adjacent if an
    edge joins a sounding of one to a sounding of the other; the colouring is greedy in ascending sequence index, every sequence
    taking the smallest colour no adjacent, already coloured sequence holds.  Returns ``colour`` int32 [L] and ``n_colours``.
    Sequences of one colour share no edge, so given the other colours they are independent: one launch draws them all."""
    p = host(ptr).reshape(-1)
    if p.size < 1 or p.dtype.kind not in "iu":
        raise ValueError("sections: ptr must be a vector of L + 1 integers")
    ptr = check_ptr(p, int(p[-1]), empty=True)
    S, L = int(ptr[-1]), ptr.size - 1
    eu, ev = host(eu).reshape(-1), host(ev).reshape(-1)
    if eu.size != ev.size or (eu.size and (eu.dtype.kind not in "iu" or ev.dtype.kind not in "iu")):
        raise ValueError("sections.line_colours: eu and ev must hold one integer per edge")
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    if np.any(eu < 0) or np.any(ev < 0) or np.any(eu >= S) or np.any(ev >= S):
        raise ValueError("sections.line_colours: every endpoint must lie in 0 .. %d" % (S - 1))
    line = _line_of(ptr, S)
    a, b = line[eu], line[ev]
    adjacent = [set() for _ in range(L)]
    for p_, q_ in zip(a[a != b].tolist(), b[a != b].tolist()):
        adjacent[p_].add(q_)
        adjacent[q_].add(p_)
    colour = np.zeros(L, dtype=np.int32)
    for l in range(L):
        taken = {int(colour[q]) for q in adjacent[l] if q < l}
        c = 0
        while c in taken:
            c += 1
        colour[l] = c
    return colour, int(colour.max(initial=-1)) + 1


def cross_incoming(eu, ev, cross, n_soundings):
    """The CSR of every sounding's incoming CROSS directed edges (numpy int32): ``cross_ptr`` [S + 1] and ``cross_edge``, ids 2 e
    (eu[e] -> ev[e]) and 2 e + 1 (ev[e] -> eu[e]) of the edges with ``cross`` [E] set, sorted by the sounding they come from."""
    at = np.flatnonzero(cross).astype(np.int64)
    src, dst = np.concatenate([eu[at], ev[at]]).astype(np.int64), np.concatenate([ev[at], eu[at]]).astype(np.int64)
    ids = np.concatenate([2 * at, 2 * at + 1])
    order = np.lexsort((src, dst))
    cross_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=int(n_soundings)))]).astype(np.int32)
    return cross_ptr, ids[order].astype(np.int32)


def _check_graph_draw(eu, ev, g, d2, n_used, score, ptr, n_draws, seed, sweeps, row_key, state, first_sweep, what):
    """The host checks ``graph_draw`` and its reference share, in the project's order (shapes, dtypes, values).  Returns eu, ev, n_used
    (numpy int64), ptr, step_edge, cross, R, seed, sweeps, first_sweep, the keys (int64 [S]) and the states to continue from (int32
    [R, S] or None)."""
    eu, ev, nu, _, _ = _check_graph(eu, ev, g, d2, n_used, score, 1, 0.0, what)
    S = nu.size
    ptr, step_edge, cross = check_lines(eu, ev, ptr, S, what)
    R = check_int(n_draws, 1, MAX_DRAWS, "%s: n_draws" % what)
    seed = _check_seed(seed)
    sweeps = check_int(sweeps, 0, MAX_DRAW_SWEEPS, "%s: sweeps" % what)
    first_sweep = check_int(first_sweep, 0, sweeps, "%s: first_sweep (at most sweeps)" % what)
    key = _check_row_key(row_key, S, what)
    if (state is None) != (first_sweep == 0):
        raise ValueError("%s: state holds the states to continue from: it goes with first_sweep > 0, and only with it" % what)
    if state is not None:
        state = host(state)
        if state.shape != (R, S) or state.dtype.kind not in "iu":
            raise ValueError("%s: state must hold one integer per realisation and sounding [%d, %d]" % (what, R, S))
        if np.any(state < 0) or np.any(state >= nu[None, :]):
            raise ValueError("%s: every state must lie in 0 .. n_used - 1" % what)
        state = state.astype(np.int32)
    return eu, ev, nu, ptr, step_edge, cross, R, seed, sweeps, first_sweep, key, state


def graph_draw_reference(eu, ev, g, d2, n_used, ptr, n_draws, seed=0, sweeps=8, score=None, row_key=None, state=None, first_sweep=0,
                         dtype=np.float64):
    """The rule of ``graph_draw`` in numpy, evaluated in ``dtype``: R joint realisations of the whole graph of ``propagate_reference``
    by Gibbs sampling blocked by flight line.  The graph as there (``eu`` < ``ev`` sorted, ``g`` [E], ``d2`` [E, n, n],
    ``n_used`` [S] in 1 .. n, ``score`` [S, n] or None); ``ptr`` [L + 1]: the sequences in the same numbering, contiguous, possibly
    empty; ``n_draws`` = R in 1 .. 65536; ``seed`` (uint64); ``sweeps`` = T >= 0; ``row_key`` int64 [S] (None: the index).

    Edges.  An edge with ev = eu + 1 inside one sequence is a *step*; every other edge must join two different sequences: a *cross*
    edge.  An edge inside a sequence that is not a step is refused, and so is a sequence in which a consecutive pair is not an edge
    (cut ``ptr`` there; ``neighbours`` produces neither).  A sequence of one sounding is legal: with L = S singletons the scheme is
    chromatic single-site Gibbs.  Colours: ``line_colours``.  K_e = exp(-(g[e] * d2[e])) on the prefixes, w_s = exp(score_s).

    Sweep 0, the start: every sequence alone -- ``draw_reference`` word for word, cross edges ignored, the uniform
    ``philox_uniform(seed, rho, row_key[s], sweep=0)``.
    Sweep t = 1 .. T: colours ascending; for every sequence of the colour and every realisation rho the same filter and walk with w'
    in place of w: w'_s[i] = w_s[i] times, for every cross edge of s in ascending order of the neighbour q, K_e[i, x_q] if s = eu[e]
    or K_e[x_q, i] if s = ev[e], x_q the neighbour's current state in realisation rho, the multiplies left to right.  The step matrix
    is K of the step edge; the uniform is ``philox_uniform(seed, rho, row_key[s], sweep=t)``.  States are replaced in place; the
    sequences of a colour read only states of other colours.
    ``first_sweep`` > 0 continues from ``state`` int32 [R, S] and runs the sweeps first_sweep .. T.

    Every line update leaves the joint law invariant, so the chain's stationary law is the *exact* joint, loops included -- where the
    beliefs of ``propagate`` are an approximation.  The R realisations are independent chains of T sweeps from the line-alone start:
    draws of the joint only as far as T sweeps have mixed.  T = 8 is a convention, not a measured mixing time.

    Returns ``draw_state`` int32 [R, S] after sweep T, ``filtered`` [R, S, n] (the alpha of the last sweep in which each sounding was
    drawn; 0.0 for the states >= m_s) and ``margin`` [R, S]: the smallest, over the sweeps run, of ``draw_reference``'s margin."""
    ft = np.dtype(dtype).type
    what = "sections.graph_draw_reference"
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    eu, ev, nu, ptr, step_edge, cross, R, seed, T, first, key, state = _check_graph_draw(eu, ev, g, d2, n_used, score, ptr, n_draws, seed, sweeps,
                                                                                         row_key, state, first_sweep, what)
    E, n, S = d2.shape[0], d2.shape[1], nu.size
    g64 = np.asarray(host(g), dtype=np.float64).reshape(-1)
    score64 = np.zeros((S, n)) if score is None else score
    rho = np.arange(R, dtype=np.int64)
    X = np.zeros((R, S), dtype=np.int32) if state is None else state.copy()
    filtered, margin = np.zeros((R, S, n), dtype=ft), np.full((R, S), np.inf, dtype=ft)
    if first == 0:                                                            # the start: the chains of the steps alone
        has = step_edge >= 0
        gc, dc = np.ones(S), np.zeros((S, n, n))
        gc[has], dc[has] = g64[step_edge[has]], d2[step_edge[has]]
        start = draw_reference(ptr, score64, gc, dc, nu, R, seed=seed, row_key=key, dtype=dtype)
        X[:], filtered[:], margin[:] = start["draw_state"], start["filtered"][None, :, :], start["margin"]
    if T < max(first, 1):
        return dict(draw_state=X, filtered=filtered, margin=margin)
    gq = g64.astype(ft)
    w = [np.exp(score64[s, :nu[s]].astype(ft)) for s in range(S)]
    K = [np.exp(-(gq[e] * d2[e, :nu[eu[e]], :nu[ev[e]]].astype(ft))) for e in range(E)]
    cross_ptr, cross_edge = cross_incoming(eu, ev, cross, S)
    colour, n_colours = line_colours(eu, ev, ptr)

    def conditioned(s):
        """w' [R, m_s] under the current states."""
        v = np.repeat(w[s][None, :], R, axis=0)
        for d in cross_edge[cross_ptr[s]:cross_ptr[s + 1]]:                   # ascending neighbour
            e = int(d) >> 1
            v = v * (K[e][:, X[:, ev[e]]].T if d & 1 else K[e][X[:, eu[e]], :])
        return np.ascontiguousarray(v)

    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(max(first, 1), T + 1):
            for c in range(n_colours):
                for l in np.flatnonzero(colour == c):
                    r0, N = int(ptr[l]), int(ptr[l + 1] - ptr[l])
                    if N == 0:
                        continue
                    m = [int(v) for v in nu[r0:r0 + N]]
                    alpha = [None] * N
                    v = conditioned(r0)
                    alpha[0] = v / v.sum(axis=1)[:, None]
                    for s in range(N - 1):
                        Ks = K[step_edge[r0 + s]]
                        u = np.zeros((R, m[s + 1]), dtype=ft)
                        for i in range(m[s]):                                # i ascending
                            u = u + alpha[s][:, i, None] * Ks[i][None, :]
                        u = np.ascontiguousarray(conditioned(r0 + s + 1) * u)
                        alpha[s + 1] = u / u.sum(axis=1)[:, None]
                    j, new = None, np.zeros((R, N), dtype=np.int32)
                    for s in range(N - 1, -1, -1):
                        filtered[:, r0 + s, :m[s]] = alpha[s]
                        W = alpha[s] if s == N - 1 else alpha[s] * K[step_edge[r0 + s]][:, j].T
                        cs = np.cumsum(np.ascontiguousarray(W), axis=1, dtype=ft)      # sequential, i ascending
                        thr = philox_uniform(seed, rho, key[r0 + s], sweep=t).astype(ft) * cs[:, -1]
                        j = np.minimum((cs <= thr[:, None]).sum(axis=1), m[s] - 1)
                        margin[:, r0 + s] = np.minimum(margin[:, r0 + s], np.abs(cs - thr[:, None]).min(axis=1) / cs[:, -1])
                        new[:, s] = j
                    X[:, r0:r0 + N] = new
    return dict(draw_state=X, filtered=filtered, margin=margin)


def graph_log_score(draw_state, score, g, d2, eu, ev):
    """f64 [R]: the log score sum_s score[s, x_s] - sum_e g[e] d2[e, x_u, x_v] of every realisation ``draw_state`` [R, S], by gathers in
    torch on the device of ``d2`` (``score`` None: zeros; ``g``, ``eu``, ``ev`` tensors there)."""
    x = draw_state.long()
    R, S = x.shape
    out = torch.zeros(R, dtype=torch.float64, device=x.device)
    if score is not None and S:
        out = score[torch.arange(S, device=x.device)[None, :], x].sum(dim=1)
    if d2.shape[0]:
        out = out - (g[None, :] * d2[torch.arange(d2.shape[0], device=x.device)[None, :], x[:, eu.long()], x[:, ev.long()]]).sum(dim=1)
    return out


def graph_draw(d2, g, eu, ev, n_used, ptr, n_draws, seed=0, sweeps=8, score=None, row_key=None, kernel=None, state=None, first_sweep=0,
               block=None, budget_bytes=4 << 30, trace=False, filtered=True):
    """R joint realisations of the whole survey graph on the device by Gibbs sampling blocked by flight line (gbp_section_graph_draw:
    csrc/gbp_section_graph_draw.h; ``graph_draw_reference`` states the rule and what its draws are).  ``d2`` f64 [E, n, n] on the
    device, n <= 256; ``g``, ``eu``, ``ev``, ``n_used`` as ``propagate`` takes them; ``ptr`` [L + 1] (host): the sequences; ``n_draws``
    = R in 1 .. 65536, ``seed`` a uint64, ``sweeps`` = T in 0 .. 65535 (8 is a convention, not a measured mixing time), ``score`` f64
    [S, n] on the device or None, ``row_key`` int64 [S] (None: the index).  ``kernel``: the K = exp(-(g d2)) that
    ``propagate(..., keep_kernel=True)`` left for the same graph; the entry then reads neither g nor d2.  ``first_sweep`` > 0 continues
    from ``state`` int32 [R, S] (host or device).  Realisations are independent chains whose random numbers depend on (seed,
    realisation, key, sweep): they are processed in blocks of ``block`` (None: as many as keep the block's alpha, R_b S n 8 bytes,
    under ``budget_bytes``), and the blocking changes no draw.

    Returns on the device ``draw_state`` int32 [R, S] and, with ``filtered``, ``filtered`` f64 [R, S, n] (then the blocks are slices
    of it).  ``trace`` runs sweep by sweep and adds ``log_score_trace`` f64 [T - first_sweep + 1, R] (the log score
    ``graph_log_score`` after every sweep that was run: T + 1 rows from the start, the start included) and ``change_share`` f64
    [T - max(first_sweep, 1) + 1]: the share of (realisation, sounding) pairs whose state a conditioned sweep changed -- how a user
    looks at mixing.  There is no host fallback."""
    entry, what = "gbp_section_graph_draw", "sections.graph_draw"
    given = (d2,) + tuple(a for a in (score, kernel) if a is not None)
    are_tensors(given, "sections", "graph_draw", entry)
    eu, ev, nu, ptr, step_edge, cross, R, seed, T, first, key, state = _check_graph_draw(eu, ev, g, d2, n_used, score, ptr, n_draws, seed, sweeps,
                                                                                         None if row_key is None else row_key, state, first_sweep, what)
    if kernel is not None and tuple(kernel.shape) != tuple(d2.shape):
        raise ValueError("%s: kernel must have the shape of d2" % what)
    if any(a.dtype != torch.float64 for a in given):
        raise TypeError("%s: d2, score and kernel are float64" % what)
    check_block(block, what)
    budget_bytes = check_int(budget_bytes, 1, 2 ** 62, "%s: budget_bytes" % what)
    on_device(given, "sections", "graph_draw", entry)
    dev = d2.device
    E, n, S, L = d2.shape[0], d2.shape[1], nu.size, ptr.size - 1
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    per = int(block) if block is not None else max(1, min(R, budget_bytes // max(1, S * n * 8)))
    per = min(per, R)
    out = dict(draw_state=torch.zeros((R, S), **i32) if state is None else torch.as_tensor(state).to(dev).contiguous())
    alpha = torch.zeros((R if filtered else per, S, n), **f64)
    if filtered:
        out["filtered"] = alpha
    run_first = max(first, 1)
    if trace:
        out.update(log_score_trace=torch.zeros((T - first + 1, R), **f64), change_share=torch.zeros(max(T - run_first + 1, 0), **f64))
    if S == 0:
        return out
    colour, n_colours = line_colours(eu, ev, ptr)
    order = np.argsort(colour, kind="stable")
    colour_ptr = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))])
    cross_ptr, cross_edge = cross_incoming(eu, ev, cross, S)
    to = lambda a, t=np.int32: torch.as_tensor(np.ascontiguousarray(a, dtype=t)).to(dev)      # noqa: E731
    t_eu, t_ev, t_nu, t_step, t_cptr, t_colptr, t_colline = (to(a) for a in (eu, ev, nu, step_edge, cross_ptr, colour_ptr, order))
    t_cedge = to(np.concatenate([cross_edge, [-1]]))                           # (never empty: the entry refuses a NULL pointer)
    t_ptr, t_key = to(ptr, np.int64), None if row_key is None else to(key, np.int64)
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev) if not torch.is_tensor(g) else g.to(dev, torch.float64).reshape(-1).contiguous()
    d2 = d2.contiguous()
    t_score = torch.zeros((S, n), **f64) if score is None else score.contiguous()
    K = torch.empty_like(d2) if kernel is None else kernel.contiguous()
    ready = kernel is not None
    w, scale = torch.empty((S, n), **f64), torch.empty((per, S), **f64)
    X = out["draw_state"]
    for a, b in ([(t, t) for t in range(first, T + 1)] if trace else [(first, T)]):
        before = X.clone() if trace and a >= 1 else None
        for r0 in range(0, R, per):
            r1 = min(R, r0 + per)
            _lib.call(entry, dev, S, E, n, L, t_ptr, t_eu, t_ev, t_nu, t_score, t_g, d2, int(ready), K, t_step, t_cptr, t_cedge, n_colours, t_colptr,
                      t_colline, t_key, seed, r1 - r0, r0, a, b, w, alpha[r0:r1] if filtered else alpha[:r1 - r0], scale, X[r0:r1])
        ready = True
        if trace:
            out["log_score_trace"][a - first] = graph_log_score(X, None if score is None else t_score, t_g, d2, t_eu, t_ev)
            if before is not None:
                out["change_share"][a - run_first] = (X != before).double().mean()
    return out


# ---- across lines: the most probable section by max-sum message passing ---------------------------------------------

MAX_REFINE = 65536
MAX_CANDIDATES = 65536
PATH_KEYS = ("sweeps", "damping", "refine")


def _first_above(v):
    """(position, value) of the first maximum of ``v`` from -inf, replaced on strict >: a NaN never wins, and without an entry above
    -inf the result is (0, -inf)."""
    ok = v > -np.inf
    if not ok.any():
        return 0, v.dtype.type(-np.inf)
    i = int(np.argmax(np.where(ok, v, -np.inf)))                              # the first of equal maxima
    return i, v[i]


def _check_edges(eu, ev, n_soundings, what):
    S = check_int(n_soundings, 0, 2 ** 31 - 1, "%s: n_soundings" % what)
    eu, ev = host(eu).reshape(-1), host(ev).reshape(-1)
    if eu.size != ev.size or (eu.size and (eu.dtype.kind not in "iu" or ev.dtype.kind not in "iu")):
        raise ValueError("%s: eu and ev must hold one integer per edge" % what)
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    if np.any(eu < 0) or np.any(ev >= S) or np.any(eu >= ev) or np.any(np.diff(eu * S + ev) <= 0):
        raise ValueError("%s: the edges need 0 <= eu < ev < %d, sorted by (eu, ev) without duplicates" % (what, S))
    return eu, ev, S


def _neighbour_lists(eu, ev, S):
    """Per sounding the directed edges that come in (ascending neighbour) and the neighbours they come from."""
    in_ptr, in_edge = incoming(eu, ev, S)
    src = np.empty(2 * eu.size, dtype=np.int64)
    src[0::2], src[1::2] = eu, ev
    inc = [in_edge[in_ptr[s]:in_ptr[s + 1]] for s in range(S)]
    return inc, src


def decode_levels(eu, ev, n_soundings):
    """The order in which ``graph_path`` decides the soundings (host, numpy): ``level`` int32 [S], the breadth-first level of every
    sounding counted from the lowest index of its connected piece (that sounding has level 0), neighbours visited in ascending order;
    ``level_ptr`` int32 [n_levels + 1] and ``level_node`` int32 [S], the soundings sorted by level (ascending index within one).  On a
    forest every sounding of level l > 0 has exactly one neighbour of a lower level, its parent."""
    eu, ev, S = _check_edges(eu, ev, n_soundings, "sections.decode_levels")
    inc, src = _neighbour_lists(eu, ev, S)
    level = np.full(S, -1, dtype=np.int32)
    for root in range(S):
        if level[root] >= 0:
            continue
        level[root] = 0
        queue, at = [root], 0
        while at < len(queue):
            s = queue[at]
            at += 1
            for q in src[inc[s]]:
                if level[q] < 0:
                    level[q] = level[s] + 1
                    queue.append(int(q))
    level_ptr = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=1 if S else 0))]).astype(np.int32)
    return level, level_ptr, np.argsort(level, kind="stable").astype(np.int32)


def sounding_colours(eu, ev, n_soundings):
    """A colouring of the soundings (host, numpy) for the coordinate ascent of ``refine``: greedy in ascending index, every sounding
    taking the smallest colour no lower-indexed neighbour holds.  Returns ``colour`` int32 [S] and ``n_colours``.  Soundings of one
    colour share no edge, so moving them together is moving them one after the other."""
    eu, ev, S = _check_edges(eu, ev, n_soundings, "sections.sounding_colours")
    inc, src = _neighbour_lists(eu, ev, S)
    colour = np.zeros(S, dtype=np.int32)
    for s in range(S):
        taken = {int(colour[q]) for q in src[inc[s]] if q < s}
        c = 0
        while c in taken:
            c += 1
        colour[s] = c
    return colour, int(colour.max(initial=-1)) + 1


def _colour_lists(eu, ev, S):
    """``colour_ptr`` int32 [n_colours + 1] and ``colour_node`` int32 [S]: the soundings sorted by colour."""
    colour, n_colours = sounding_colours(eu, ev, S)
    colour_ptr = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))]).astype(np.int32)
    return colour_ptr, np.argsort(colour, kind="stable").astype(np.int32)


def _check_states(state, nu, most, what, name):
    """``state`` (host or device) as numpy int32 [R, S] with every entry in 0 .. n_used - 1; also whether it came as one row [S]."""
    x = host(state)
    single = x.ndim == 1
    x = x[None, :] if single else x
    if x.ndim != 2 or x.shape[1] != nu.size or x.dtype.kind not in "iu" or not 1 <= x.shape[0] <= most:
        raise ValueError("%s: %s must hold one integer per sounding, [S] or [R, S] with S = %d and 1 <= R <= %d" % (what, name, nu.size, most))
    if np.any(x < 0) or np.any(x >= nu[None, :]):
        raise ValueError("%s: every entry of %s must lie in 0 .. n_used - 1" % (what, name))
    return np.ascontiguousarray(x, dtype=np.int32), single


def _path_terms(eu, ev, g, d2, nu, score):
    """theta_s on the prefix (zeros without a score) and c_e = g[e] * d2[e] on the prefixes, one multiply."""
    g = np.asarray(host(g), dtype=np.float64).reshape(-1)
    theta = [np.zeros(nu[s]) if score is None else score[s, :nu[s]].copy() for s in range(nu.size)]
    return theta, [g[e] * d2[e, :nu[eu[e]], :nu[ev[e]]] for e in range(eu.size)]


def _cost_to(c, d, x):
    """The costs of the states of the sounding directed edge ``d`` ends in, its source at state ``x``: 2 e + 1 comes from ev[e] into
    eu[e] (column x of c_e), 2 e from eu[e] into ev[e] (row x)."""
    return c[d >> 1][:, x] if d & 1 else c[d >> 1][x, :]


def _refine_rule(X, theta, c, eu, ev, sweeps):
    """Coordinate ascent of one section ``X`` int32 [S], in place; returns the moves of every sweep, int32 [sweeps]."""
    S = X.size
    inc, src = _neighbour_lists(eu, ev, S)
    colour, n_colours = sounding_colours(eu, ev, S)
    moves = np.zeros(sweeps, dtype=np.int32)
    for t in range(sweeps):
        for col in range(n_colours):
            for s in np.flatnonzero(colour == col):                           # (they share no edge: together is one after the other)
                v = theta[s].copy()
                for d in inc[s]:                                              # ascending neighbour
                    v = v - _cost_to(c, int(d), X[src[d]])
                i, top = _first_above(v)
                if top > v[X[s]]:
                    X[s] = i
                    moves[t] += 1
        if moves[t] == 0:
            break
    return moves


def _host_log_score(X, score, g, d2, eu, ev):
    """``graph_log_score`` of numpy states on the host."""
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt))      # noqa: E731
    return graph_log_score(t(X, np.int32), None if score is None else t(score, np.float64), t(host(g).reshape(-1), np.float64), t(d2, np.float64),
                           t(eu, np.int64), t(ev, np.int64)).numpy()


def refine_reference(state, eu, ev, g, d2, n_used, score=None, sweeps=16):
    """The rule of ``refine`` in numpy: coordinate ascent on the exact log score sum_s score[s, x_s] - sum_e g[e] d2[e, x_u, x_v] of
    the sections ``state`` int [S] or [R, S] on the graph of ``propagate_reference``.  ``sounding_colours`` colours the soundings; a
    sweep visits the colours in ascending order and the soundings of a colour together.  For sounding s, v[i] = theta_s[i] (the score,
    0.0 without one) minus c_e at (x_q, i) for every neighbour q in ascending order, c_e = g[e] * d2[e]; s moves to the first maximum
    of v over i < m_s (from -inf on strict >) only if v there is strictly greater than v[x_s]: every move raises the score, and a NaN
    moves nothing.  A section stops after a sweep without a move or after ``sweeps`` sweeps.

    Returns ``state`` int32 (the shape given), ``refine_moves`` int32 [R, sweeps] ([sweeps] for one section) and ``log_score`` f64 [R]
    (a number for one section; ``graph_log_score``)."""
    what = "sections.refine_reference"
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    eu, ev, nu, _, _ = _check_graph(eu, ev, g, d2, n_used, score, 1, 0.0, what)
    sweeps = check_int(sweeps, 0, MAX_REFINE, "%s: sweeps" % what)
    X, single = _check_states(state, nu, MAX_CANDIDATES + 1, what, "state")
    X = X.copy()
    theta, c = _path_terms(eu, ev, g, d2, nu, score)
    with np.errstate(invalid="ignore"):
        moves = np.stack([_refine_rule(X[r], theta, c, eu, ev, sweeps) for r in range(X.shape[0])])
    ls = _host_log_score(X, score, g, d2, eu, ev)
    return dict(state=X[0] if single else X, refine_moves=moves[0] if single else moves, log_score=ls[0] if single else ls)


def graph_path_reference(eu, ev, g, d2, n_used, score=None, sweeps=32, damping=0.0, refine=16, candidates=None):
    """The rule of ``graph_path`` in numpy (fp64: what the device is held to, bit for bit): the most probable section of the graph of
    ``propagate_reference`` -- the same arguments -- by synchronous max-sum message passing, a decode by conditioning and coordinate
    ascent.  Everything is in the log domain; there is no exp.

    Terms.  theta_s[i] = score[s, i] (None: 0.0); c_e[i, j] = g[e] * d2[e, i, j], one multiply.  Directed edge 2 e is u -> v through
    c_e, 2 e + 1 is v -> u through its transpose; the message nu[d] has m_dst entries and starts at 0.0.
    A sweep computes every message from the last sweep's.  For a -> b: h[i] = theta_a[i] + nu[c -> a][i] over the neighbours c != b of
    a, ascending c; u[j] = the maximum over i < m_a of h[i] - c[i, j], from -inf and replaced on strict >, so a NaN candidate never
    wins (the convention of ``track_reference``); top = the maximum of u by the same loop; nu' = u - top: the largest entry is 0.0.  A
    message with no candidate above -inf is NaN through (-inf) - (-inf), as a zero total is in ``propagate_reference``.  With
    ``damping`` = lam != 0 nu' = (1 - lam) nu' + lam nu_old.  ``residual[t]`` is the largest |nu' - nu_old| of sweep t (NaN if a
    message is; 0.0 without edges).
    ``max_marginal`` [S, n] = theta_s plus all incoming messages (ascending neighbour), minus its maximum; -inf for the states >= m_s.
    On a tree, once the sweeps have reached its diameter, max_marginal[s, i] is exactly the log probability lost by forcing sounding s
    onto model i.
    Decode.  ``decode_levels`` gives every sounding a breadth-first level; the levels decide in ascending order, the soundings of a level
    together: x_s = the first maximum over i < m_s of theta_s[i] plus, per neighbour q ascending, -c at (x_q, i) if level(q) <
    level(s), else nu[q -> s][i].  On a forest every sounding then conditions on exactly one decided neighbour, its parent, and the
    decode is a mode whatever the ties -- where the argmax of the max-marginals sounding by sounding mixes equal modes.  On a graph
    with loops it is an approximation.
    Refine and choose.  The decode and every row of ``candidates`` (int [C, S], states in 0 .. n_used - 1; None: none) are refined by
    ``refine`` sweeps of ``refine_reference``; the result is the refined candidate whose ``graph_log_score`` is the first maximum:
    never less probable than any candidate given.

    Returns ``state`` int32 [S], ``log_score``, ``max_marginal`` [S, n], ``residual`` [sweeps], ``decoded_state`` int32 [S] (before the
    refinement), ``candidate_state`` int32 [C + 1, S] (refined; row 0 from the decode), ``candidate_log_score`` [C + 1], ``chosen`` and
    ``refine_moves`` int32 [C + 1, refine]."""
    what = "sections.graph_path_reference"
    d2 = np.asarray(d2, dtype=np.float64)
    score = None if score is None else np.asarray(score, dtype=np.float64)
    eu, ev, nu, sweeps, damping = _check_graph(eu, ev, g, d2, n_used, score, sweeps, damping, what)
    refine = check_int(refine, 0, MAX_REFINE, "%s: refine" % what)
    given = None if candidates is None else _check_states(candidates, nu, MAX_CANDIDATES, what, "candidates")[0]
    E, n, S = d2.shape[0], d2.shape[1], nu.size
    theta, c = _path_terms(eu, ev, g, d2, nu, score)
    inc, src = _neighbour_lists(eu, ev, S)
    dst = np.empty(2 * E, dtype=np.int64)
    dst[0::2], dst[1::2] = ev, eu
    msg = [np.zeros(nu[dst[d]]) for d in range(2 * E)]
    residual = np.zeros(sweeps)
    with np.errstate(invalid="ignore"):
        for t in range(sweeps):
            new, r = [], 0.0
            for d in range(2 * E):
                a, b = int(src[d]), int(dst[d])
                h = theta[a].copy()
                for q in inc[a]:                                             # ascending neighbour
                    if src[q] != b:
                        h = h + msg[q]
                cd = c[d // 2] if d % 2 == 0 else c[d // 2].T
                u = np.full(nu[b], -np.inf)
                for i in range(nu[a]):                                       # i ascending, strict >
                    cand = h[i] - cd[i]
                    u = np.where(cand > u, cand, u)
                m = u - _first_above(u)[1]
                if damping != 0.0:
                    m = (1.0 - damping) * m + damping * msg[d]
                r = _nan_max(r, np.abs(m - msg[d]).max())
                new.append(m)
            msg = new
            residual[t] = r
        max_marginal = np.full((S, n), -np.inf)
        for s in range(S):
            b = theta[s].copy()
            for q in inc[s]:
                b = b + msg[q]
            max_marginal[s, :nu[s]] = b - _first_above(b)[1]
        level, level_ptr, level_node = decode_levels(eu, ev, S)
        decoded = np.zeros(S, dtype=np.int32)
        for l in range(level_ptr.size - 1):
            picks = []
            for s in level_node[level_ptr[l]:level_ptr[l + 1]]:
                v = theta[s].copy()
                for d in inc[s]:
                    q = src[d]
                    v = v - _cost_to(c, int(d), decoded[q]) if level[q] < level[s] else v + msg[d]
                picks.append(_first_above(v)[0])
            decoded[level_node[level_ptr[l]:level_ptr[l + 1]]] = picks
        X = decoded[None, :].copy() if given is None else np.concatenate([decoded[None, :], given])
        moves = np.stack([_refine_rule(X[r], theta, c, eu, ev, refine) for r in range(X.shape[0])])
    ls = _host_log_score(X, score, g, d2, eu, ev)
    chosen = _first_above(ls)[0]
    return dict(state=X[chosen].copy(), log_score=ls[chosen], max_marginal=max_marginal, residual=residual, decoded_state=decoded, candidate_state=X,
                candidate_log_score=ls, chosen=chosen, refine_moves=moves)


def _graph_on_device(eu, ev, nu, g, d2, score, dev):
    """The tensors the graph entries share: eu, ev, n_used (int32), g, d2, score (zeros without one) and the CSR of incoming edges."""
    S, n = nu.size, d2.shape[1]
    in_ptr, in_edge = incoming(eu, ev, S)
    t_g = torch.as_tensor(host(g).reshape(-1).astype(np.float64)).to(dev) if not torch.is_tensor(g) else g.to(dev, torch.float64).reshape(-1).contiguous()
    t_eu, t_ev, t_nu = (torch.as_tensor(a.astype(np.int32)).to(dev) for a in (eu, ev, nu))
    t_score = torch.zeros((S, n), dtype=torch.float64, device=dev) if score is None else score.contiguous()
    return t_eu, t_ev, t_nu, t_score, t_g, d2.contiguous(), torch.as_tensor(in_ptr).to(dev), torch.as_tensor(in_edge).to(dev)


def _refine_on_device(X, graph, eu, ev, sweeps):
    """gbp_section_graph_refine on the sections ``X`` int32 [C, S] (device, contiguous), in place; returns the moves int32 [C, sweeps]."""
    t_eu, t_ev, t_nu, t_score, t_g, d2, t_ptr, t_edge = graph
    C, S = X.shape
    moves = torch.zeros((C, sweeps), dtype=torch.int32, device=X.device)
    if S == 0 or sweeps == 0:
        return moves
    colour_ptr, colour_node = _colour_lists(eu, ev, S)
    _lib.call("gbp_section_graph_refine", X.device, S, t_eu.numel(), d2.shape[1], C, t_eu, t_ev, t_nu, t_score, t_g, d2, t_ptr, t_edge, colour_ptr.size - 1,
              np.ctypeslib.as_ctypes(colour_ptr), torch.as_tensor(colour_node).to(X.device), sweeps, X, moves)
    return moves


def _check_path_device(d2, score, module_what, entry):
    if d2.dtype != torch.float64 or (score is not None and score.dtype != torch.float64):
        raise TypeError("sections.%s: d2 and score are float64" % module_what)
    on_device((d2,) + (() if score is None else (score,)), "sections", module_what, entry)


def refine(state, d2, g, eu, ev, n_used, score=None, sweeps=16):
    """Coordinate ascent on the exact log score on the device (gbp_section_graph_refine: csrc/gbp_section_graph_path.h
    k_graph_condition; ``refine_reference`` states the rule): the sections ``state`` int [S] or [R, S] (host or device; R <= 65537)
    on the graph ``d2`` f64 [E, n, n] on the device, ``g``, ``eu``, ``ev``, ``n_used``, ``score`` as ``propagate`` takes them, move
    sounding by sounding to their best state given their neighbours until a sweep moves nothing or ``sweeps`` sweeps are done.  What
    comes back is a local mode of the joint: it polishes a decode, and takes Gibbs draws of ``graph_draw`` to the modes they sit under.
    Returns on the device ``state`` int32 (the shape given), ``refine_moves`` int32 [R, sweeps] ([sweeps] for one section) and
    ``log_score`` f64 [R] (0-d for one section).  There is no host fallback."""
    entry, what = "gbp_section_graph_refine", "sections.refine"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "refine", entry)
    eu, ev, nu, _, _ = _check_graph(eu, ev, g, d2, n_used, score, 1, 0.0, what)
    sweeps = check_int(sweeps, 0, MAX_REFINE, "%s: sweeps" % what)
    X, single = _check_states(state, nu, MAX_CANDIDATES + 1, what, "state")
    _check_path_device(d2, score, "refine", entry)
    dev = d2.device
    graph = _graph_on_device(eu, ev, nu, g, d2, score, dev)
    X = torch.as_tensor(X).to(dev)
    moves = _refine_on_device(X, graph, eu, ev, sweeps)
    ls = graph_log_score(X, None if score is None else graph[3], graph[4], graph[5], graph[0], graph[1])
    return dict(state=X[0] if single else X, refine_moves=moves[0] if single else moves, log_score=ls[0] if single else ls)


def graph_path(d2, g, eu, ev, n_used, n_soundings, score=None, sweeps=32, damping=0.0, refine=16, candidates=None):
    """The most probable section of the graph of ``propagate`` on the device (gbp_section_graph_path and gbp_section_graph_refine:
    csrc/gbp_section_graph_path.h; ``graph_path_reference`` states the rule, and the device has its bits): ``d2`` f64 [E, n, n] on the
    device, n <= 256; ``g``, ``eu``, ``ev``, ``n_used``, ``n_soundings``, ``score``, ``sweeps`` and ``damping`` as ``propagate`` takes
    them -- max-sum sweeps in place of sum-product ones, on d2 itself: no buffer of its size is made.  The decode is refined by up to
    ``refine`` sweeps of coordinate ascent, and so is every row of ``candidates`` (int [C, S], host or device; None: none); the
    refined section of the highest ``graph_log_score`` is returned.  Exact on a forest once the sweeps reach its diameter
    (``residual`` is then 0.0); on loops a documented approximation, never below any candidate given.

    Returns on the device ``state`` int32 [S], ``log_score`` f64 (0-d), ``max_marginal`` f64 [S, n] (-inf for the states >= n_used),
    ``residual`` f64 [sweeps], ``decoded_state`` int32 [S], ``candidate_state`` int32 [C + 1, S], ``candidate_log_score`` f64 [C + 1],
    ``refine_moves`` int32 [C + 1, refine], and ``chosen``, an integer.  The levels of the decode and the colours of the refinement are
    made once on the host; the decode takes one launch per breadth-first level."""
    entry, what = "gbp_section_graph_path", "sections.graph_path"
    are_tensors((d2,) + (() if score is None else (score,)), "sections", "graph_path", entry)
    S = check_int(n_soundings, 0, 2 ** 31 - 1, "%s: n_soundings" % what)
    if np.size(host(n_used)) != S:
        raise ValueError("%s: n_used must hold one integer per sounding (%d)" % (what, S))
    eu, ev, nu, sweeps, damping = _check_graph(eu, ev, g, d2, n_used, score, sweeps, damping, what)
    refine = check_int(refine, 0, MAX_REFINE, "%s: refine" % what)
    given = None if candidates is None else _check_states(candidates, nu, MAX_CANDIDATES, what, "candidates")[0]
    _check_path_device(d2, score, "graph_path", entry)
    dev = d2.device
    E, n = d2.shape[0], d2.shape[1]
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    max_marginal, residual, decoded = torch.empty((S, n), **f64), torch.zeros(sweeps, **f64), torch.zeros(S, **i32)
    graph = _graph_on_device(eu, ev, nu, g, d2, score, dev)
    t_eu, t_ev, t_nu, t_score, t_g, d2, t_ptr, t_edge = graph
    if S:
        level, level_ptr, level_node = decode_levels(eu, ev, S)
        nu_buf, resid = torch.empty((2, 2 * E, n), **f64), torch.empty((sweeps, 2 * E), **f64)
        _lib.call(entry, dev, S, E, n, t_eu, t_ev, t_nu, t_score, t_g, d2, t_ptr, t_edge, sweeps, damping, level_ptr.size - 1,
                  np.ctypeslib.as_ctypes(level_ptr), torch.as_tensor(level_node).to(dev), torch.as_tensor(level).to(dev), nu_buf, resid, max_marginal,
                  decoded, residual)
    X = decoded[None, :].clone() if given is None else torch.cat([decoded[None, :], torch.as_tensor(given).to(dev)]).contiguous()
    moves = _refine_on_device(X, graph, eu, ev, refine)
    ls = graph_log_score(X, None if score is None else t_score, t_g, d2, t_eu, t_ev)
    chosen = _first_above(ls.cpu().numpy())[0]
    return dict(state=X[chosen].clone(), log_score=ls[chosen].clone(), max_marginal=max_marginal, residual=residual, decoded_state=decoded, candidate_state=X,
                candidate_log_score=ls, chosen=chosen, refine_moves=moves)


def check_path(path, what):
    """``path`` of ``spatial`` as the keywords of ``graph_path``: None, True or a dictionary with ``sweeps``, ``damping``, ``refine``."""
    if path is None or path is False:
        return None
    if path is True:
        path = {}
    if not isinstance(path, dict) or not set(path) <= set(PATH_KEYS):
        raise ValueError("%s: path is None, True or a dictionary with %s" % (what, ", ".join(PATH_KEYS)))
    return dict(sweeps=check_int(path.get("sweeps", 32), 1, MAX_SWEEPS, "%s: path sweeps" % what), damping=_check_damping(path.get("damping", 0.0), what),
                refine=check_int(path.get("refine", 16), 0, MAX_REFINE, "%s: path refine" % what))


def spatial(ens, x, y, z1, z0=0.0, measure="linear", ptr=None, chains=1, max_models=64, *, max_distance, tau=0.1, length=100.0, min_distance=1.0,
            score=None, sweeps=32, damping=0.0, budget_bytes=4 << 30, products=None, draws=None, seed=0, draw_sweeps=8, bodies=None, boreholes=None,
            path=None):
    """One kept model per sounding, and a weight for every kept model, from the whole survey at once: the chain of
    ``sections`` along every sequence of ``ptr`` plus edges to the nearest sounding of every other sequence within ``max_distance``
    (required; about 1.5 line spacings), solved by ``sweeps`` synchronous sweeps of sum-product message passing with ``damping``.
    The pipeline is ``families.used_rows`` (``chains``, ``max_models`` <= 256), ``neighbours`` (``tau``, ``length``, ``min_distance``),
    ``edge_distance``, ``propagate`` and a gather.  Exact along a line and on any survey whose graph is a forest; with loops the
    weights are beliefs, an approximation whose size DESIGN.md 3.28 records, and ``residual`` says whether the sweeps settled.

    Returns, on the device: ``weight`` f64 [S, n] (the belief; NaN: no models), ``n_effective`` f64 [S] = 1 / sum w^2, ``state`` int32
    [S] (the first maximum of the belief, a position in ``rows``; -1: no models), ``slot`` int32 [S], ``rows`` int32 [S, n],
    ``n_used`` int32 [S], ``section_k`` / ``section_edges`` / ``section_sigma`` (bit copies of the chosen slots, as in ``sections``),
    ``edge_u`` / ``edge_v`` int32 [E], ``edge_length`` f64 [E] (m), ``edge_distance`` f64 [E] (D in decades between the chosen models
    of the edge's soundings) and ``residual`` f64 [sweeps].  ``products`` = dict(depth_edges=, percentiles=, thresholds=) adds what
    ``lateral_products`` gives under this ``weight``.  The graph is one problem and is not cut into blocks: E n^2 8 bytes of distances
    (and as much again for exp(-g D^2)) above ``budget_bytes`` are refused.

    ``draws`` = R adds R joint realisations of the whole survey (``graph_draw`` with ``seed`` and ``draw_sweeps`` sweeps, on the K of
    ``propagate``; the key of a sounding is its index in the survey before soundings without models are dropped):
    ``draw_state`` / ``draw_slot`` int32 [R, S] (-1: no models; ``draw_models`` gathers the models), ``draw_log_score`` f64 [R]
    (sum score - sum g d2 over the graph), ``draw_share`` f64 [S, n] (the frequency of every state among the draws, NaN without
    models: to be read against ``weight``, which is an approximation on loops where the draws' law is exact once mixed) and
    ``draw_change_share`` f64 [draw_sweeps] (the share of states every sweep changed).  With ``draws`` None every other output keeps
    its bits.

    ``bodies`` = dict(depth_edges=, lo=, hi=, ...) (it needs ``draws``) adds the connected bodies of the realisations on this graph,
    ``edge_u`` / ``edge_v`` (``draw_bodies``): ``body_count`` int64, ``body_largest_measure`` / ``body_member_measure``
    f64 [R, G] per connected piece of the graph (``a`` defaults to ``section_widths``: m^2; give ``bodies.sounding_areas`` for m^3) and
    ``body_largest_share`` f64 [S, C].  With None every other output keeps its bits.

    ``boreholes`` = dict(logs=, max_distance=, ...) as in ``sections`` (its ``max_distance`` is the reach of a log, not the one of the
    graph): the borehole score is added to ``score`` before the message passing and the draws, and the ``borehole_*`` outputs of
    ``sections`` are added, ``borehole_log_predictive`` under the beliefs.  With None every other output keeps its bits.

    ``path`` = True or dict(sweeps=, damping=, refine=) adds the most probable section of the whole graph (``graph_path``; DESIGN.md
    3.32) -- ``state`` is the first maximum of every sounding's belief taken alone, and neighbouring picks need not go together:
    ``path_state`` / ``path_slot`` int32 [S] (-1: no models), ``path_k`` / ``path_edges`` / ``path_sigma`` (bit copies of the chosen
    slots), ``path_log_score`` and ``state_log_score`` (``graph_log_score`` of the path and of ``state``, to compare), ``path_margin``
    f64 [S] (the gap between the two largest max-marginals: what forcing the sounding off its model costs at least; inf with one model,
    NaN without), ``path_residual`` f64 [sweeps of the path], ``path_candidate_log_score`` and ``path_chosen`` (the refined candidates:
    the decode, ``state`` and, with ``draws``, the best-scoring draw; the path is never less probable than any of them) and
    ``path_edge_distance`` f64 [E].  With None every other output keeps its bits."""
    z0, z1, _ = check_window(z0, z1, measure)
    path = check_path(path, "sections.spatial")
    if boreholes is not None:
        boreholes = _bh.check_options(boreholes, "sections.spatial")
    if products is not None:
        products = check_products(products)
    if bodies is not None:
        bodies = check_bodies(bodies, "sections.spatial")
        if draws is None:
            raise ValueError("sections.spatial: bodies are those of joint realisations; they need draws")
    R = None if draws is None else check_int(draws, 1, MAX_DRAWS, "sections.spatial: draws")
    seed, draw_sweeps = _check_seed(seed), check_int(draw_sweeps, 0, MAX_DRAW_SWEEPS, "sections.spatial: draw_sweeps")
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    are_tensors((k, edges, sigma), "sections", "spatial", "gbp_ensemble_cross_distance")
    if k.ndim != 2 or edges.ndim != 3:
        raise ValueError("ensemble: k [S, n_slots], edges and sigma [S, n_slots, K]")
    C = check_chains(chains, k.shape[1])
    max_models = check_int(max_models, 1, MAX_GRAPH_STATES, "max_models")
    budget_bytes = check_int(budget_bytes, 1, 2 ** 62, "budget_bytes")
    sweeps, damping = check_int(sweeps, 1, MAX_SWEEPS, "sweeps"), _check_damping(damping, "sections.spatial")
    S = k.shape[0]
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != S or y.size != S:
        raise ValueError("sections: x and y must hold one entry per sounding (%d)" % S)
    p = _default_ptr(ptr, S)
    max_distance = _check_number(max_distance, "max_distance")
    steps(x, y, tau, length, min_distance, p)                                  # (its refusals of x, y, tau, length and min_distance)
    rows, n_used, _ = used_rows(ens, chains=C, max_models=max_models)
    n = rows.shape[1]
    if score is not None:
        are_tensors((score,), "sections", "spatial", "gbp_section_propagate")
        if tuple(score.shape) != (S, n) or score.dtype != torch.float64:
            raise ValueError("sections: score must be float64 [S, n] with n = %d, the width of used_rows" % n)
    nu = host(n_used).reshape(-1).astype(np.int64)
    eu, ev, g, dist = neighbours(x, y, p, nu, max_distance=max_distance, tau=tau, length=length, min_distance=min_distance)
    E = eu.size
    if E * n * n * 8 > budget_bytes:
        raise ValueError("sections.spatial: %d edges with %d models a sounding need %d bytes of distances, more than budget_bytes = %d; lower "
                         "max_models or max_distance, or raise budget_bytes (the graph is one problem: it is not cut into blocks)"
                         % (E, n, E * n * n * 8, budget_bytes))
    on_device((k, edges, sigma) + (() if score is None else (score,)), "sections", "spatial", "gbp_ensemble_cross_distance")
    if boreholes is not None:
        b_score, b_att, b_part, b_skipped = _bh.section_score(ens, rows, n_used, x, y, p, boreholes, tau, length)
        score = b_score if score is None else score + b_score
    dev = k.device
    f64 = dict(dtype=torch.float64, device=dev)
    d2 = edge_distance(ens, rows, eu, ev, z0, z1, measure=measure)
    keep = np.flatnonzero(nu > 0)
    local = np.cumsum(nu > 0) - 1                                              # the soundings with models, renumbered: the order stays
    idx = torch.as_tensor(keep).to(dev)
    res = propagate(d2, g, local[eu], local[ev], nu[keep], keep.size, score=None if score is None else score[idx], sweeps=sweeps, damping=damping,
                    keep_kernel=R is not None)
    nan = float("nan")
    weight, state = torch.full((S, n), nan, **f64), torch.full((S,), -1, dtype=torch.int32, device=dev)
    weight[idx], state[idx] = res["belief"], res["state"]
    has = state >= 0
    w = torch.where(has[:, None], weight, torch.zeros((), **f64))
    out = dict(weight=weight, n_effective=torch.where(has, 1.0 / (w * w).sum(dim=1), torch.full((), nan, **f64)))
    out.update(_chosen_models(k, edges, sigma, rows, n_used, state))
    t_u, t_v = torch.as_tensor(eu.astype(np.int64)).to(dev), torch.as_tensor(ev.astype(np.int64)).to(dev)
    st = state.long()
    out.update(edge_u=t_u.to(torch.int32), edge_v=t_v.to(torch.int32), edge_length=torch.as_tensor(dist).to(dev),
               edge_distance=torch.sqrt(d2[torch.arange(E, device=dev), st[t_u], st[t_v]]), residual=res["residual"])
    if R is not None:
        _, piece_ptr, _ = pieces(p, nu)                                        # the runs of soundings with models: the sequences of the graph
        drawn = graph_draw(d2, g, local[eu], local[ev], nu[keep], piece_ptr, R, seed=seed, sweeps=draw_sweeps, score=None if score is None else score[idx],
                           row_key=keep, kernel=res["kernel"], budget_bytes=budget_bytes, trace=True, filtered=False)
        draw_state = torch.full((R, S), -1, dtype=torch.int32, device=dev)
        draw_state[:, idx] = drawn["draw_state"]
        dl = draw_state.long().clamp(min=0)
        dslot = torch.gather(rows.long()[None, :, :].expand(R, S, n), 2, dl[:, :, None])[:, :, 0].clamp(min=0)
        share = torch.zeros((S, n), **f64).scatter_add_(1, dl.t().contiguous(), torch.ones((S, R), **f64)) / R
        out.update(draw_state=draw_state, draw_slot=torch.where(draw_state >= 0, dslot, torch.full_like(dslot, -1)).to(torch.int32),
                   draw_log_score=drawn["log_score_trace"][-1].clone(), draw_share=torch.where(has[:, None], share, torch.full((), nan, **f64)),
                   draw_change_share=drawn["change_share"])
    if path is not None:
        l_score, l_u, l_v = None if score is None else score[idx], torch.as_tensor(local[eu]).to(dev), torch.as_tensor(local[ev]).to(dev)
        t_g = torch.as_tensor(g).to(dev)
        given = [res["state"]]                                                 # today's section, and the best realisation drawn
        if R is not None:
            given.append(drawn["draw_state"][int(torch.argmax(drawn["log_score_trace"][-1]))])
        found = graph_path(d2, g, local[eu], local[ev], nu[keep], keep.size, score=l_score, candidates=torch.stack(given), **path)
        path_state = torch.full((S,), -1, dtype=torch.int32, device=dev)
        path_state[idx] = found["state"]
        models = _chosen_models(k, edges, sigma, rows, n_used, path_state)
        two = torch.topk(found["max_marginal"], min(2, n), dim=1).values
        margin = torch.full((S,), nan, **f64)
        margin[idx] = two[:, 0] - two[:, 1] if n > 1 else torch.full((keep.size,), float("inf"), **f64)
        ps = path_state.long()
        out.update(path_state=path_state, path_slot=models["slot"], path_k=models["section_k"], path_edges=models["section_edges"],
                   path_sigma=models["section_sigma"], path_log_score=found["log_score"],
                   state_log_score=graph_log_score(res["state"][None, :], l_score, t_g, d2, l_u, l_v)[0], path_margin=margin,
                   path_residual=found["residual"], path_candidate_log_score=found["candidate_log_score"],
                   path_chosen=torch.tensor(found["chosen"], dtype=torch.int32, device=dev),
                   path_edge_distance=torch.sqrt(d2[torch.arange(E, device=dev), ps[t_u], ps[t_v]]))
    if boreholes is not None:
        out.update(_bh.section_outputs(b_att, b_score, b_part, b_skipped, weight, n_used))
    if products is not None:
        out.update(lateral_products(ens, out, **products))
    if bodies is not None:
        out.update(_body_products(ens, out["draw_slot"], x, y, p, dict(bodies, eu=eu, ev=ev)))
    return out


def line_ptr(line):
    """ptr int64 [L + 1] of the runs of consecutive rows with equal ``line`` number."""
    line = np.asarray(line).reshape(-1)
    cut = np.flatnonzero(line[1:] != line[:-1]) + 1 if line.size else np.zeros(0, dtype=np.int64)
    return np.concatenate([[0], cut, [line.size]]).astype(np.int64) if line.size else np.zeros(1, dtype=np.int64)


def _survey_ensemble(result_or_path, device, what):
    """The survey result (or the file its ``save`` wrote) and the ensemble it carries, on ``device`` (default cuda:0)."""
    from .survey import SurveyResult
    res = SurveyResult.load(result_or_path) if isinstance(result_or_path, (str, bytes)) or hasattr(result_or_path, "__fspath__") else result_or_path
    missing = [name for name in ("ensemble_k", "ensemble_edges", "ensemble_sigma", "line", "x", "y") if name not in res]
    if missing:
        raise ValueError("sections.%s: the survey result holds no %s (survey.infer(..., ensemble=n_keep) keeps the models)" % (what, ", ".join(missing)))
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    k = torch.as_tensor(np.ascontiguousarray(res["ensemble_k"], dtype=np.int32))
    e, s = (torch.as_tensor(np.ascontiguousarray(res[name], dtype=np.float64)) for name in ("ensemble_edges", "ensemble_sigma"))
    if dev.type == "cuda":
        k, e, s = k.to(dev), e.to(dev), s.to(dev)
    return res, Ensemble(k, e, s, None, None, 1, None)


def _survey_columns(res, S):
    return dict(line=np.asarray(res["line"]), fiducial=np.asarray(res["fiducial"]) if "fiducial" in res else np.arange(S),
                x=np.asarray(res["x"]), y=np.asarray(res["y"]))


SPATIAL_SHARED = ("z0", "measure", "chains", "tau", "length", "min_distance")


def _survey_boreholes(kw, res, what):
    """``kw`` with its ``boreholes`` made ready for a survey: ``logs`` may be a path, and ``surface`` defaults to the survey's
    ``elevation`` when it has one and every collar is finite (a log without a collar is read as depths below the sounding's ground)."""
    if kw.get("boreholes") is None:
        return kw
    options = kw["boreholes"]
    if not isinstance(options, dict) or "logs" not in options:
        raise ValueError("sections.%s: boreholes is a dictionary with logs and max_distance" % what)
    options = dict(options, logs=_bh.load(options["logs"]))
    if options.get("surface") is None and "elevation" in res and np.all(np.isfinite(options["logs"].collar)):
        options["surface"] = np.asarray(res["elevation"], dtype=np.float64).reshape(-1)
    return dict(kw, boreholes=options)


def _spatial_of_lines(ens, res, z1, **kw):
    return spatial(ens, res["x"], res["y"], z1, ptr=line_ptr(res["line"]), **_survey_boreholes(kw, res, "spatial_from_survey"))


def from_survey(result_or_path, z1, device=None, spatial=None, **kw):
    """``sections`` for a ``survey.SurveyResult`` -- or the file its ``save`` wrote -- that carries the kept models (``survey.infer(...,
    ensemble=...)``: ensemble_k / _edges / _sigma).  The sequences are the runs of consecutive rows with equal line number; ``kw``: the
    keywords of ``sections`` but ``ptr``.  Returns its dictionary on ``device`` (default cuda:0) plus ``line``, ``fiducial``, ``x``, ``y``
    (numpy, as stored).  ``spatial`` = dict(max_distance=..., ...) adds the result of ``spatial_from_survey`` -- the survey solved as
    one graph -- as ``spatial_<name>``: the dictionary holds keywords of ``spatial`` (``max_distance`` is required), and ``z0``,
    ``measure``, ``chains``, ``tau``, ``length`` and ``min_distance`` are taken from ``kw`` unless it names them.  ``boreholes`` (in
    ``kw``, and in ``spatial`` for the graph): its ``logs`` may be a path of ``boreholes.load``, and its ``surface`` defaults to the
    survey's ``elevation`` when it has one and every collar is finite."""
    if spatial is not None and (not isinstance(spatial, dict) or "max_distance" not in spatial or "ptr" in spatial):
        raise ValueError("sections.from_survey: spatial is a dictionary of keywords of sections.spatial with max_distance, without ptr")
    if "ptr" in kw:
        raise ValueError("sections.from_survey: the sequences are the survey's lines; ptr is not taken")
    res, ens = _survey_ensemble(result_or_path, device, "from_survey")
    out = sections(ens, res["x"], res["y"], z1, ptr=line_ptr(res["line"]), **_survey_boreholes(kw, res, "from_survey"))
    if spatial is not None:
        across = _spatial_of_lines(ens, res, z1, **dict({name: kw[name] for name in SPATIAL_SHARED if name in kw}, **spatial))
        out.update({"spatial_" + name: v for name, v in across.items()})
    out.update(_survey_columns(res, ens.k.shape[0]))
    return out


def spatial_from_survey(result_or_path, z1, device=None, **kw):
    """``spatial`` for a ``survey.SurveyResult`` or its saved file: the sequences are the survey's lines; ``kw``: the keywords of
    ``spatial`` but ``ptr`` (``max_distance`` is required).  Returns its dictionary plus ``line``, ``fiducial``, ``x``, ``y``."""
    if "ptr" in kw:
        raise ValueError("sections.spatial_from_survey: the sequences are the survey's lines; ptr is not taken")
    if "max_distance" not in kw:
        raise ValueError("sections.spatial_from_survey: max_distance is required (about 1.5 line spacings)")
    res, ens = _survey_ensemble(result_or_path, device, "spatial_from_survey")
    out = _spatial_of_lines(ens, res, z1, **kw)
    out.update(_survey_columns(res, ens.k.shape[0]))
    return out


def fit_ensemble(ens, x, y, z1, z0=0.0, measure="linear", ptr=None, chains=1, max_models=128, length=100.0, min_distance=1.0, tau_max=0.8,
                 rungs=11, spatial=None):
    """``fit_tau`` for an ensemble, on the plumbing of ``sections``: ``families.used_rows`` (``chains``, ``max_models``), ``steps``
    at ``tau_max``, ``pieces`` (a sequence is cut at soundings without models), ``cross_distance`` and the fit.  ``spatial`` =
    dict(max_distance=, sweeps=, damping=) fits on the survey graph instead (``neighbours``, ``edge_distance``, ``fit_tau_graph``;
    ``max_models`` <= 256).  The distances of the whole survey are held at once: S n^2 8 bytes (E n^2 8 for the graph).  Returns the
    dictionary of ``fit_tau`` (``fit_tau_graph``)."""
    z0, z1, _ = check_window(z0, z1, measure)
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    are_tensors((k, edges, sigma), "sections", "fit_ensemble", "gbp_ensemble_cross_distance")
    if k.ndim != 2 or edges.ndim != 3:
        raise ValueError("ensemble: k [S, n_slots], edges and sigma [S, n_slots, K]")
    if spatial is not None and (not isinstance(spatial, dict) or "max_distance" not in spatial or set(spatial) - {"max_distance", "sweeps", "damping"}):
        raise ValueError("sections.fit_ensemble: spatial is a dictionary with max_distance and, optionally, sweeps and damping")
    tau_max, rungs = _check_fit(tau_max, rungs, "sections.fit_ensemble")
    C = check_chains(chains, k.shape[1])
    max_models = check_int(max_models, 1, MAX_STATES if spatial is None else MAX_GRAPH_STATES, "max_models")
    S = k.shape[0]
    x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    if x.size != S or y.size != S:
        raise ValueError("sections: x and y must hold one entry per sounding (%d)" % S)
    p = _default_ptr(ptr, S)
    g = steps(x, y, tau_max, length, min_distance, p)
    rows, n_used, _ = used_rows(ens, chains=C, max_models=max_models)
    on_device((k, edges, sigma), "sections", "fit_ensemble", "gbp_ensemble_cross_distance")
    dev = k.device
    nu = host(n_used).reshape(-1).astype(np.int64)
    if spatial is not None:
        eu, ev, g, _ = neighbours(x, y, p, nu, max_distance=spatial["max_distance"], tau=tau_max, length=length, min_distance=min_distance)
        d2 = edge_distance(ens, rows, eu, ev, z0, z1, measure=measure)
        keep = np.flatnonzero(nu > 0)
        local = np.cumsum(nu > 0) - 1                                          # the soundings with models, renumbered: the order stays
        return fit_tau_graph(d2, g, local[eu], local[ev], nu[keep], keep.size, tau0=tau_max, tau_max=tau_max, rungs=rungs,
                             sweeps=spatial.get("sweeps", 32), damping=spatial.get("damping", 0.0))
    keep, piece_ptr, _ = pieces(p, nu)
    idx = torch.as_tensor(keep).to(dev)
    partner = np.arange(1, keep.size + 1, dtype=np.int32)
    partner[piece_ptr[1:] - 1] = -1
    sub = Ensemble(k[idx], edges[idx], sigma[idx], None, None, ens.thin, None)
    d2 = cross_distance(sub, rows[idx], partner, z0, z1, measure=measure, squared=True)
    return fit_tau(d2, g[keep], piece_ptr, nu[keep], tau0=tau_max, tau_max=tau_max, rungs=rungs)


def fit_from_survey(result_or_path, z1, device=None, spatial=None, **kw):
    """``fit_ensemble`` for a ``survey.SurveyResult`` or its saved file: the sequences are the survey's lines; ``kw``: the keywords of
    ``fit_ensemble`` but ``ptr``; ``spatial`` = dict(max_distance=, ...) fits on the survey graph."""
    if "ptr" in kw:
        raise ValueError("sections.fit_from_survey: the sequences are the survey's lines; ptr is not taken")
    res, ens = _survey_ensemble(result_or_path, device, "fit_from_survey")
    return fit_ensemble(ens, res["x"], res["y"], z1, ptr=line_ptr(res["line"]), spatial=spatial, **kw)


def output_path(path, suffix=OUTPUT_SUFFIX):
    """<name>.sections.npz (``suffix``) beside the survey result <name>.npz."""
    path = str(path)
    return (path[:-4] if path.endswith(".npz") else path) + suffix


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def _parser():
    import argparse
    from .families import MEASURES
    p = argparse.ArgumentParser(prog="python -m geobipy_amd.sections",
                                description="One kept model per sounding, chosen jointly along every flight line of a saved survey result that "
                                            "carries its ensemble; writes <name>.sections.npz")
    p.add_argument("survey", help="a survey result written by SurveyResult.save (.npz) with ensemble_k / _edges / _sigma")
    p.add_argument("--depth", type=float, required=True, metavar="Z1", help="the bottom of the depth window (m)")
    p.add_argument("--from", dest="z0", type=float, default=0.0, metavar="Z0", help="the top of the depth window (default 0)")
    p.add_argument("--measure", choices=MEASURES, default="linear", help="weigh depth linearly or by its logarithm (log needs --from > 0)")
    p.add_argument("--tau", type=float, default=None, metavar="T", help="decades of RMS difference per --length metres (default 0.1)")
    p.add_argument("--fit-tau", type=float, nargs="*", default=None, metavar="TAU_MAX [RUNGS]",
                   help="learn tau from the sections themselves first (the zero of the evidence's derivative over a ladder of RUNGS values from "
                        "TAU_MAX downward by sqrt 2; default 0.8 11; with --spatial on the survey graph) and use it for everything else; adds "
                        "fit_tau, fit_tau_sd_log, fit_tau_ladder and fit_log_evidence; not together with --tau")
    p.add_argument("--length", type=float, default=100.0, metavar="L", help="the distance --tau refers to, m (default 100)")
    p.add_argument("--max-models", type=int, default=128, metavar="n", help="the most models per sounding, 1 .. 1024 (default 128)")
    p.add_argument("--chains", type=int, default=1, metavar="C", help="replicate chains on the slot axis (default 1)")
    p.add_argument("--no-marginals", action="store_true", help="only the path: skip the forward-backward pass")
    p.add_argument("--draws", type=int, default=0, metavar="R", help="joint realisations of every line to draw, 0 .. 65536 (default 0: none)")
    p.add_argument("--seed", type=int, default=0, metavar="N", help="the seed of the draws, a uint64 (default 0)")
    p.add_argument("--depth-axis", nargs=2, metavar=("N", "WIDTH"), default=None,
                   help="add the laterally weighted posterior on N uniform cells of WIDTH starting at 0: lateral_mean, lateral_sd, "
                        "lateral_percentile_<p>, lateral_exceedance")
    p.add_argument("--percentiles", type=float, nargs="+", default=None, metavar="P", help="with --depth-axis: ascending percentiles in [0, 100] (default 5 50 95)")
    p.add_argument("--exceed", type=float, nargs="+", default=None, metavar="T", help="with --depth-axis: at most 8 thresholds in log10 S/m (default none)")
    p.add_argument("--spatial", type=float, default=None, metavar="MAX_DISTANCE",
                   help="solve the survey as one graph: join every sounding to the nearest one of every other line within MAX_DISTANCE metres "
                        "(about 1.5 line spacings) and write <name>.spatial.npz instead (--max-models <= 256)")
    p.add_argument("--sweeps", type=int, default=None, metavar="N", help="with --spatial: sweeps of message passing (default 32)")
    p.add_argument("--damping", type=float, default=None, metavar="L", help="with --spatial: the damping of the messages in [0, 1) (default 0)")
    p.add_argument("--spatial-draws", type=int, default=None, metavar="R",
                   help="with --spatial: joint realisations of the whole survey to draw, 1 .. 65536 (uses --seed); adds draw_state, draw_slot, "
                        "draw_log_score, draw_share and draw_change_share")
    p.add_argument("--draw-sweeps", type=int, default=None, metavar="T", help="with --spatial-draws: Gibbs sweeps over the lines (default 8)")
    p.add_argument("--path", type=int, nargs="?", const=True, default=None, metavar="SWEEPS",
                   help="with --spatial: the most probable section of the whole graph by SWEEPS sweeps of max-sum message passing (default 32), "
                        "refined by coordinate ascent; adds path_state, path_slot, path_k, path_edges, path_sigma, path_log_score, state_log_score, "
                        "path_margin, path_residual, path_candidate_log_score, path_chosen and path_edge_distance")
    p.add_argument("--bodies", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="with --depth-axis and --draws (or --spatial-draws): the connected bodies of the realisations' cells with LO <= log10 S/m "
                        "<= HI (a bound far outside, such as -99 or 99: none); adds body_count, body_largest_measure, body_member_measure and body_largest_share")
    p.add_argument("--boreholes", default=None, metavar="LOGS",
                   help="condition on borehole logs: a file of geobipy_amd.boreholes (.npz, or the text table name,x,y,collar,top,bottom,value,sd,"
                        "class); needs --borehole-distance; adds borehole_score, borehole_sounding, borehole_index, borehole_distance, "
                        "borehole_skipped and borehole_log_predictive")
    p.add_argument("--borehole-distance", type=float, default=None, metavar="D",
                   help="with --boreholes: attach a log to the nearest sounding of every line within D metres")
    p.add_argument("--class-means", type=float, nargs="+", default=None, metavar="M", help="with --boreholes: the class means of lithology intervals, log10 S/m")
    p.add_argument("--class-scales", type=float, nargs="+", default=None, metavar="S", help="with --boreholes: as many class scales, decades")
    p.add_argument("--class-floor", type=float, default=None, metavar="F",
                   help="with --boreholes: the probability that a lithology entry says nothing, in (0, 1) (default 1e-6)")
    p.add_argument("--device", default="cuda:0")
    return p


def parse_args(argv=None):
    """The command line as (path, keywords of ``from_survey``); refuses before any device work."""
    p = _parser()
    a = p.parse_args(argv)
    fit = None
    if a.fit_tau is not None:
        if a.tau is not None:
            p.error("--fit-tau learns tau: it is not given together with --tau")
        if len(a.fit_tau) > 2 or (len(a.fit_tau) == 2 and a.fit_tau[1] != int(a.fit_tau[1])):
            p.error("--fit-tau [TAU_MAX [RUNGS]]: a number and an integer")
        try:
            fit = dict(zip(("tau_max", "rungs"), _check_fit(a.fit_tau[0] if a.fit_tau else 0.8, int(a.fit_tau[1]) if len(a.fit_tau) == 2 else 11, "--fit-tau")))
        except ValueError as e:
            p.error(str(e))
    if a.tau is None:
        a.tau = 0.1
    try:
        check_window(a.z0, a.depth, a.measure)
        _check_number(a.tau, "--tau")
        _check_number(a.length, "--length")
        check_int(a.chains, 1, 8, "--chains")
        check_int(a.max_models, 1, MAX_STATES, "--max-models")
        check_int(a.draws, 0, MAX_DRAWS, "--draws")
        _check_seed(a.seed)
    except ValueError as e:
        p.error(str(e))
    kw = dict(z1=a.depth, z0=a.z0, measure=a.measure, tau=a.tau, length=a.length, max_models=a.max_models, chains=a.chains,
              marginals=not a.no_marginals, device=a.device)
    if a.draws:
        kw.update(draws=a.draws, seed=a.seed)
    if a.boreholes is None:
        if a.borehole_distance is not None or a.class_means is not None or a.class_scales is not None or a.class_floor is not None:
            p.error("--borehole-distance, --class-means, --class-scales and --class-floor need --boreholes")
    else:
        if a.borehole_distance is None:
            p.error("--boreholes needs --borehole-distance D (the reach of a log is not guessed)")
        if (a.class_means is None) != (a.class_scales is None):
            p.error("--class-means and --class-scales are given together")
        try:
            _check_number(a.borehole_distance, "--borehole-distance")
            if a.class_means is not None:
                from .line_products import check_classes
                check_classes(a.class_means, a.class_scales)
            if a.class_floor is not None and not 0.0 < a.class_floor < 1.0:
                raise ValueError("--class-floor must lie in (0, 1)")
        except ValueError as e:
            p.error(str(e))
        kw["boreholes"] = dict(logs=a.boreholes, max_distance=a.borehole_distance,
                               classes=None if a.class_means is None else (tuple(a.class_means), tuple(a.class_scales)),
                               class_floor=1e-6 if a.class_floor is None else a.class_floor)
    if a.bodies is not None and not (a.draws if a.spatial is None else a.spatial_draws):
        p.error("--bodies labels joint realisations: it needs --draws R (or --spatial D --spatial-draws R)")
    if a.depth_axis is None:
        if a.percentiles is not None or a.exceed is not None:
            p.error("--percentiles and --exceed need --depth-axis")
        if a.bodies is not None:
            p.error("--bodies needs --depth-axis (the cells the bodies are made of)")
    else:
        try:
            n, w = int(a.depth_axis[0]), float(a.depth_axis[1])
        except ValueError:
            p.error("--depth-axis N WIDTH: an integer and a number")
        if n < 1 or not (np.isfinite(w) and w > 0.0):
            p.error("--depth-axis: N >= 1 and a finite, positive WIDTH")
        if a.no_marginals:
            p.error("--depth-axis needs the marginals (drop --no-marginals)")
        try:
            kw["products"] = check_products(dict(depth_edges=np.arange(n + 1, dtype=np.float64) * w,
                                                 percentiles=(5, 50, 95) if a.percentiles is None else a.percentiles,
                                                 thresholds=() if a.exceed is None else a.exceed))
        except ValueError as e:
            p.error("--" + str(e))
        if a.bodies is not None:
            try:
                kw["bodies"] = check_bodies(dict(depth_edges=np.arange(n + 1, dtype=np.float64) * w, lo=a.bodies[0], hi=a.bodies[1]), "--bodies")
            except ValueError as e:
                p.error(str(e))
    if a.spatial is None:
        if a.sweeps is not None or a.damping is not None or a.spatial_draws is not None or a.path is not None:
            p.error("--sweeps, --damping, --spatial-draws and --path need --spatial")
        if a.draw_sweeps is not None:
            p.error("--draw-sweeps needs --spatial-draws")
    else:
        if a.no_marginals or a.draws:
            p.error("--spatial takes neither --no-marginals nor --draws (the draws of single lines); joint draws of the survey are --spatial-draws")
        if a.draw_sweeps is not None and a.spatial_draws is None:
            p.error("--draw-sweeps needs --spatial-draws")
        try:
            if a.spatial_draws is not None:
                check_int(a.spatial_draws, 1, MAX_DRAWS, "--spatial-draws")
            if a.draw_sweeps is not None:
                check_int(a.draw_sweeps, 0, MAX_DRAW_SWEEPS, "--draw-sweeps")
            _check_number(a.spatial, "--spatial")
            check_int(a.max_models, 1, MAX_GRAPH_STATES, "--max-models (with --spatial)")
            if a.sweeps is not None:
                check_int(a.sweeps, 1, MAX_SWEEPS, "--sweeps")
            if a.damping is not None:
                _check_damping(a.damping, "--damping")
            if a.path is not None and a.path is not True:
                check_int(a.path, 1, MAX_SWEEPS, "--path")
        except ValueError as e:
            p.error(str(e))
        del kw["marginals"]
        if a.path is not None:
            kw["path"] = True if a.path is True else dict(sweeps=a.path)
        kw.update(max_distance=a.spatial, **({} if a.sweeps is None else dict(sweeps=a.sweeps)), **({} if a.damping is None else dict(damping=a.damping)))
        if a.spatial_draws is not None:
            kw.update(draws=a.spatial_draws, seed=a.seed, **({} if a.draw_sweeps is None else dict(draw_sweeps=a.draw_sweeps)))
    if fit is not None:
        kw["fit_tau"] = fit                                                   # (``main`` takes it out again: no keyword of ``from_survey``)
    return a.survey, kw


def _fit_for_main(path, kw):
    """The fit the command line runs first: on the lines, or with --spatial on the survey graph, with the window, measure, chains,
    max-models, length, sweeps and damping of the invocation.  Returns the keywords with ``tau`` = tau_hat and what the output file gets."""
    fit_kw = kw.pop("fit_tau")
    shared = {name: kw[name] for name in ("z0", "measure", "chains", "max_models", "length", "device") if name in kw}
    across = dict(max_distance=kw["max_distance"], **{name: kw[name] for name in ("sweeps", "damping") if name in kw}) if "max_distance" in kw else None
    fit = fit_from_survey(path, kw["z1"], spatial=across, **shared, **fit_kw)
    factor = float(np.exp(fit["tau_sd_log"]))
    print("fit: tau = %.4g decades per %g m, error factor %s, %s" % (fit["tau"], kw["length"], "%.3f" % factor if np.isfinite(factor) else "unknown",
                                                                      "bracketed" if fit["bracketed"] else "NOT bracketed: the ladder's end"))
    stored = dict(fit_tau=np.float64(fit["tau"]), fit_tau_sd_log=np.float64(fit["tau_sd_log"]), fit_tau_ladder=np.asarray(fit["tau_ladder"]),
                  fit_log_evidence=np.asarray(fit["log_evidence"]))
    return dict(kw, tau=fit["tau"]), stored


def main(argv=None):
    path, kw = parse_args(argv)
    if "fit_tau" in kw:
        kw, stored = _fit_for_main(path, kw)
        result = spatial_from_survey(path, **kw) if "max_distance" in kw else from_survey(path, **kw)
        result.update(stored)
        out = save(result, output_path(path, SPATIAL_SUFFIX if "max_distance" in kw else OUTPUT_SUFFIX))
        print("wrote", out)
        return out
    if "max_distance" in kw:
        out = save(spatial_from_survey(path, **kw), output_path(path, SPATIAL_SUFFIX))
    else:
        out = save(from_survey(path, **kw), output_path(path))
    print("wrote", out)
    return out


if __name__ == "__main__":
    main()
