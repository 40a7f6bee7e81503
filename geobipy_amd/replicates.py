"""Replicate chains: C rjMCMC chains per sounding, their posteriors pooled into one and their agreement mapped per depth cell
(csrc/gbp_hitmap.h k_hitmap_pool).  The reference runs one chain per sounding and has no counterpart, so the rule is
stated here on the host (``pool_reference``) and the kernel is held to it.

The sampler needs no change: ``DeviceChains(chain_id=...)`` keys every chain's random streams, and ``expand`` gives replicate c of the
sounding in row r of the data file the id r + c n_file -- replicate 0 walks the chain the sounding walks alone.  ``Pooled`` then shows a
finished block of S C chains as S soundings: histograms summed over the chains that burned in, per-chain state from the chain with the
highest posterior.  All replicates of a sounding start from the same half-space (the reference's initialisation is deterministic) and
differ by their random streams only: R-hat from identically started chains is optimistic.
"""
import numpy as np
import torch

LN2 = 0.6931471805599453

# histogram-type chain state: summed over the used chains (the hit map goes through the kernel, the rest are small)
SUMMED = ("k_hist", "edge_hist", "rel_hist", "add_hist", "height_hist", "unit_hist", "first_hist", "first_none",
          "data_hist", "misfit_hist", "ens_seen")
# the posterior ensemble [rows, n_keep, ...]: a sounding's is the concatenation over its C chains, [S, C * n_keep, ...] in chain order,
# with ens_k = 0 (empty) in the slots of the chains that are not used
ENSEMBLE = ("ens_k", "ens_edges", "ens_sigma", "ens_misfit")
# per-chain state [rows, ...] a pooled view shows, taken from the representative chain: what survey_run.SurveyRun's run_block / summaries / payload and
# unit_posteriors.products read (the sampler's working state -- Jacobians, Cholesky factors, proposals -- is not part of the view)
PER_CHAIN = ("chain_id", "data", "observed", "height", "height0", "best_height", "log_mean_prior", "k", "edges", "sigma", "rel", "add", "prior",
             "like", "misfit", "n_accepted", "burned_in_iteration", "status", "best_posterior", "best_k", "best_edges", "best_sigma", "best_rel",
             "best_add", "best_iteration", "iteration0", "trace_misfit", "trace_accept", "unit_z", "data_scale", "misfit_scale")
# chain state every row shares (not per chain: DeviceChains.infer's re-packing leaves them alone too)
SHARED = ("add_scale", "rel_group", "add_group")


def expand(rows, C, n_file):
    """(row, chain_id), each int64 [len(rows) * C], sounding-major: ``row`` repeats every entry of ``rows`` (rows of the data file) C
    times, ``chain_id`` = row + c * n_file for replicate c, with ``n_file`` the data file's sounding count: unique over the file and
    the replicates, and replicate 0 keeps the id the sounding has without replicates."""
    rows = np.asarray(rows, dtype=np.int64).ravel()
    C, n_file = int(C), int(n_file)
    if C < 1:
        raise ValueError("expand: C = %d" % C)
    if rows.size and (rows.min() < 0 or rows.max() >= n_file):
        raise ValueError("expand: rows outside the data file's %d soundings" % n_file)
    row = np.repeat(rows, C)
    return row, row + np.tile(np.arange(C, dtype=np.int64), rows.size) * n_file


def pool_reference(maps, C, use=None, half_width=1.0):
    """The rule of ``hitmap.pool`` on the host, in numpy (the kernel's operations in the kernel's order: sequential sums along the value
    axis through ``np.cumsum(...)[-1]``, sums over the chains in ascending c).  ``maps`` [S * C, n_value, n_depth] integers, ``use``
    [S, C] or None.  Returns the dict of ``hitmap.pool`` as numpy arrays."""
    h = np.asarray(maps).astype(np.int64)
    C = int(C)
    R, nv, nz = h.shape
    assert 2 <= C <= 8 and R % C == 0
    S = R // C
    h = h.reshape(S, C, nv, nz)
    on = np.ones((S, C), dtype=bool) if use is None else (np.asarray(use).reshape(S, C) != 0)
    hw = float(half_width)
    x = ((np.arange(nv, dtype=np.float64) + 0.5) / float(nv)) * (2.0 * hw) - hw
    xv = x[None, None, :, None]
    last = lambda terms, axis: np.cumsum(terms, axis=axis).take(-1, axis=axis)      # noqa: E731  (a sequential sum, first cell first)
    hf = h.astype(np.float64)
    hx = hf * xv
    n = h.sum(axis=2)                                                   # [S, C, nz] int64
    a = last(hx, 2)
    q = last(hx * xv, 2)
    hlogh = lambda c: np.where(c > 0, c.astype(np.float64) * np.log(np.where(c > 0, c, 1).astype(np.float64)), 0.0)      # noqa: E731
    e = last(hlogh(h), 2)
    hp = (h * on[:, :, None, None]).sum(axis=1)                          # [S, nv, nz]
    ep = last(hlogh(hp), 1)
    member = on[:, :, None] & (n > 0)                                   # P
    m = member.sum(axis=1)
    with np.errstate(all="ignore"):
        nf = n.astype(np.float64)
        mc = np.where(member, a / nf, np.nan)
        s2 = np.where(n >= 2, np.maximum(0.0, (q - a * mc) / (n - 1).astype(np.float64)), 0.0)
        sw, sm, NP = np.zeros((S, nz)), np.zeros((S, nz)), np.zeros((S, nz), dtype=np.int64)
        for c in range(C):
            sw = sw + np.where(member[:, c], s2[:, c], 0.0)
            sm = sm + np.where(member[:, c], mc[:, c], 0.0)
            NP = NP + np.where(member[:, c], n[:, c], 0)
        md, Nd = m.astype(np.float64), NP.astype(np.float64)
        W, mbar = sw / md, sm / md
        sb, sj = np.zeros((S, nz)), np.zeros((S, nz))
        for c in range(C):
            d = mc[:, c] - mbar
            sb = sb + np.where(member[:, c], d * d, 0.0)
            sj = sj + np.where(member[:, c], (nf[:, c] / Nd) * (np.log(nf[:, c]) - e[:, c] / nf[:, c]), 0.0)
        Bn, nbar = sb / (m - 1).astype(np.float64), Nd / md
        rhat = np.where(W == 0.0, np.where(Bn == 0.0, 1.0, np.inf), np.sqrt(((nbar - 1.0) / nbar * W + Bn) / W))
        jsd = np.maximum(0.0, ((np.log(Nd) - ep / Nd) - sj) / LN2)
    few = m < 2
    return dict(pooled=hp.astype(np.int32), n_used=m.astype(np.int32), chain_mean=mc, rhat=np.where(few, np.nan, rhat),
                jsd=np.where(few, np.nan, jsd))


class Pooled:
    """A finished block of S * C chains (row s * C + c: replicate c of sounding s) seen as S soundings: the names ``survey_run.SurveyRun`` (run_block, summaries, payload) and
    ``unit_posteriors.products`` / ``data_posteriors.products`` read of a sampler -- ``t`` (the chain state by the names of gbp_rj_chains),
    ``hitmap``, ``unit_hist``, ``first_hist``, ``first_none``, ``data_hist``, ``misfit_hist``, ``ens_k`` ... (``ENSEMBLE``), ``observed``, ``B`` -- and the sampler's own attributes for the rest.  ``t`` holds the names of
    ``PER_CHAIN``, ``SUMMED`` and ``SHARED`` (None where the sampler has none), not the sampler's working state.

    ``use`` [S, C]: the chain burned in -- under the reference's schedule its status is not "failed" (2); without the schedule every
    chain.  Histogram-type state (``SUMMED`` and the hit map) is the sum over the used chains; every other per-chain tensor is the row
    of the sounding's representative chain, ``rep`` [S]: the used chain with the highest ``best_posterior``, the lowest c among equals,
    c = 0 when none is used.  ``dc``: a sampler, or a dict of its tensors (then ``reference_schedule`` says whether ``status`` counts:
    default, when the dict has one)."""

    def __init__(self, dc, C, reference_schedule=None):
        self.dc, self.C = dc, int(C)
        C = self.C
        if not 2 <= C <= 8:
            raise ValueError("Pooled: C = %d replicate chains, 2 .. 8 are supported" % C)
        sampler = not isinstance(dc, dict)
        if sampler and dc.t.get("hitmap") is not None:
            dc.hitmap                                  # (attribute access settles the dwell times of every posterior that has them)
        t = dc.t if sampler else dc
        rows = int(t["best_posterior"].shape[0])
        if rows % C:
            raise ValueError("Pooled: %d chains are not %d per sounding" % (rows, C))
        self.B = S = rows // C
        dev = t["best_posterior"].device
        if reference_schedule is None:
            reference_schedule = bool(dc._o.schedule == 1) if sampler else t.get("status") is not None
        use = (t["status"] != 2) if reference_schedule else torch.ones(rows, dtype=torch.bool, device=dev)
        self.use = use = use.view(S, C)
        score = torch.where(use, t["best_posterior"].view(S, C), torch.full((), float("-inf"), dtype=torch.float64, device=dev))
        c_idx = torch.arange(C, device=dev)[None, :].expand(S, C)
        first = torch.where(score == score.max(dim=1, keepdim=True).values, c_idx, torch.full_like(c_idx, C)).min(dim=1).values
        self.rep = rep = torch.where(first < C, first, torch.zeros_like(first))
        self.rep_rows = rep_rows = torch.arange(S, device=dev) * C + rep
        self.half_width = float(dc.value_half_width if sampler else t.get("value_half_width", 1.0))
        self._pool, self._diagnostics = None, None
        out = {}
        for name in ENSEMBLE:
            v = t.get(name)
            if v is not None:
                v = v.view((S, C * v.shape[1]) + tuple(v.shape[2:]))
                if name == "ens_k":
                    v = v * use.to(v.dtype).repeat_interleave(v.shape[1] // C, dim=1)
            out[name] = v
        for name in PER_CHAIN + SUMMED + SHARED + ("hitmap",):
            v = t.get(name)
            if v is None or name in SHARED:
                out[name] = v
            elif name == "hitmap":
                out[name] = None                   # (pooled by the kernel on first use: ``hitmap``)
            elif name in SUMMED:
                mask = use.view((S, C) + (1,) * (v.ndim - 1)).to(v.dtype)
                out[name] = (v.view((S, C) + tuple(v.shape[1:])) * mask).sum(dim=1).to(v.dtype)
            else:
                out[name] = v[rep_rows].contiguous()
        self._maps = t.get("hitmap")
        # a column of a chain's hit map holds at most one count per sample, and every sample is one count of k_hist
        self._max_total = int(t["k_hist"].sum(dim=1, dtype=torch.int64).max()) if t.get("k_hist") is not None and rows else None
        self.t = out

    def __getattr__(self, name):
        d = self.__dict__
        if "t" not in d or "dc" not in d:
            raise AttributeError(name)
        if name in d["t"]:
            return d["t"][name]
        if isinstance(d["dc"], dict):
            raise AttributeError(name)
        return getattr(d["dc"], name)

    @property
    def observed(self):
        return self.t["observed"] if self.t.get("observed") is not None else self.t["data"]

    def pool(self):
        """The five outputs of ``hitmap.pool`` for the block's hit maps (one kernel pass, kept)."""
        if self._pool is None:
            if self._maps is None:
                raise ValueError("Pooled: the chains kept no hit map (DeviceChains(hitmap=True))")
            from . import hitmap
            self._pool = hitmap.pool(self._maps, self.C, self.use, self.half_width, max_total=self._max_total)
            self.t["hitmap"] = self._pool["pooled"]
        return self._pool

    @property
    def hitmap(self):
        return None if self._maps is None else self.pool()["pooled"]

    def diagnostics(self):
        """Convergence of the replicates: ``rhat``, ``jsd``, ``n_used`` [S, n_depth] and ``chain_mean`` [S, C, n_depth] of the hit map's
        columns (log10 conductivity about the prior mean); ``rhat_layers`` / ``jsd_layers`` [S] of the layer count (``k_hist``) and
        ``rhat_interfaces`` [S] of the interface depth (``edge_hist``), each histogram taken as a map of one column through the same
        entry (value axis scaled to +-1); ``rhat_max`` [S], the largest finite ``rhat`` of the sounding's cells (NaN when none is)."""
        if self._diagnostics is None:
            from . import hitmap
            p = self.pool()
            out = {k: p[k] for k in ("rhat", "jsd", "n_used", "chain_mean")}
            src = self.dc.t if not isinstance(self.dc, dict) else self.dc
            one = lambda name: hitmap.pool(src[name].contiguous()[:, :, None], self.C, self.use, 1.0)      # noqa: E731
            layers, interfaces = one("k_hist"), one("edge_hist")
            out["rhat_layers"], out["jsd_layers"] = layers["rhat"][:, 0], layers["jsd"][:, 0]
            out["rhat_interfaces"] = interfaces["rhat"][:, 0]
            finite = torch.isfinite(p["rhat"])
            top = torch.where(finite, p["rhat"], torch.full_like(p["rhat"], float("-inf"))).max(dim=1).values
            out["rhat_max"] = torch.where(finite.any(dim=1), top, torch.full_like(top, float("nan")))
            self._diagnostics = out
        return self._diagnostics
