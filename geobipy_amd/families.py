"""Families of kept models: which sampled model is representative, and is the posterior one family of models or several (DESIGN.md 3.23;
csrc/gbp_ensemble_families.h).

The products of ``ensembles`` are statements about depth cells.  These are statements about the kept MODELS themselves:

``distance``   the RMS difference in decades between every two kept layered models of a sounding over a depth window -- the exact
               integral of the squared difference of two piecewise-constant functions, O(k_i + k_j) per pair, no depth axis
               (gbp_ensemble_distance; ``distance_reference`` states the rule in numpy).
``cluster``    k-medoids on those distances for 1 .. ``max_families`` families, every stage in one launch (gbp_distance_families;
               ``families_reference`` states the rule: every output is an integer or a copy of an input double, so the device is held to
               it with ``==``), with the cost, the medoid-based silhouette and the family shares of every stage.
``select``     how many families: the found stage with the greatest silhouette among those that pass ``min_silhouette`` and ``min_share``.
``families``   all of the above for an ensemble: the medoid of all models (``central_*``: a kept model, not a smooth average, to hand on
               as "the" layered model of a sounding), the families of the selected stage ordered by share with their medoid models, and
               with replicate chains the share of every chain in every family (a family only one replicate visits is not converged).

``python -m geobipy_amd.families <ensemble.npz> --depth Z1 [--from Z0] [--measure log] [--chains C] [--max-families Q]`` writes
``<name>.families.npz`` for a saved ensemble.  There is no host fallback: ``distance``, ``cluster`` and ``families`` refuse tensors that
are not on the device.
"""
import numpy as np
import torch

from . import _lib
from ._args import are_tensors, check_block, check_ensemble, check_int, on_device
from .ensembles import MIN_CHAIN_COUNT, check_chains, segments  # noqa: F401  (MIN_CHAIN_COUNT: the rule ``used_rows`` shares)

MEASURES = ("linear", "log")
MAX_MODELS, MAX_FAMILIES, MAX_K = 4096, 8, 64
DISTANCE_BLOCK_BYTES = 2 << 30


def check_window(z0, z1, measure):
    """(z0, z1, index of ``measure``): finite bounds with 0 <= z0 < z1, ``measure`` "linear" or "log" (log: z0 > 0)."""
    if measure not in MEASURES:
        raise ValueError("measure must be 'linear' or 'log'")
    for v in (z0, z1):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("the window's bounds z0 and z1 are numbers")
    z0, z1 = float(z0), float(z1)
    if not (np.isfinite(z0) and np.isfinite(z1)) or z0 < 0.0 or z1 <= z0:
        raise ValueError("the window needs finite bounds with 0 <= z0 < z1")
    if measure == "log" and z0 == 0.0:
        raise ValueError("the log measure needs z0 > 0")
    return z0, z1, MEASURES.index(measure)


# ---- the rules ------------------------------------------------------------------------------------------------------------------------

def distance_reference(k, edges, sigma, rows, z0, z1, measure="linear", dtype=np.float64, stored=False, squared=False):
    """The rule of ``distance`` for one sounding, in numpy: ``k`` [n_slots], ``edges`` / ``sigma`` [n_slots, K], model u is slot
    ``rows[u]``; evaluated in ``dtype`` (np.longdouble: what the device is held to).  Returns D [n, n] (``squared``: D^2).

    A model has k layers, interfaces e[0 .. k - 2] ascending and values a[l] = log10 sigma[l] (``stored``: sigma[l] as it is); its value at
    depth z is that of layer #{l < k - 1 : e[l] <= z} (an interface exactly at z gives the layer below).  With mu([p, q]) = q - p
    (linear) or ln(q / p) (log, z0 > 0):  D^2(u, v) = (1 / mu([z0, z1])) sum over the merged segments [p, q) of mu([p, q]) (a_u(p) -
    a_v(p))^2, the breakpoints being z0, every interface of either model strictly inside (z0, z1) in ascending order, and z1; the sum
    runs in that order.  The diagonal of a present model is 0; a row outside 0 .. n_slots - 1 or a slot with k <= 0 is absent: its row,
    column and diagonal are NaN."""
    z0, z1, log = check_window(z0, z1, measure)
    k, edges, sigma = np.asarray(k), np.asarray(edges, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    rows = np.asarray(rows).reshape(-1)
    if k.ndim != 1 or edges.ndim != 2 or edges.shape != sigma.shape or edges.shape[0] != k.shape[0]:
        raise ValueError("distance_reference: k [n_slots], edges and sigma [n_slots, K]")
    n_slots, K = edges.shape
    n = rows.size
    p0, p1 = dtype(z0), dtype(z1)
    mu = (lambda p, q: np.log1p((q - p) / p)) if log else (lambda p, q: q - p)      # (ln(q / p), accurate however thin the segment)
    total = mu(p0, p1)
    models = []
    for r in rows:
        kk = min(max(int(k[r]), 0), K) if 0 <= r < n_slots else 0
        if kk == 0:
            models.append(None)
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            a = sigma[r, :kk].astype(dtype)
            models.append((edges[r, :kk - 1], a if stored else np.log10(a)))
    out = np.full((n, n), np.nan, dtype=dtype)
    for u in range(n):
        if models[u] is None:
            continue
        out[u, u] = 0
        eu, au = models[u]
        for v in range(u + 1, n):
            if models[v] is None:
                continue
            ev, av = models[v]
            inner = np.unique(np.concatenate([eu, ev]))
            bp = np.concatenate([[z0], inner[(inner > z0) & (inner < z1)], [z1]])
            p, q = bp[:-1].astype(dtype), bp[1:].astype(dtype)
            d = au[np.searchsorted(eu, bp[:-1], side="right")] - av[np.searchsorted(ev, bp[:-1], side="right")]
            with np.errstate(invalid="ignore"):
                d2 = np.cumsum(mu(p, q) * (d * d))[-1] / total              # (cumsum: the segments in ascending order)
                out[u, v] = out[v, u] = d2 if squared else np.sqrt(d2)
    return out


def families_reference(D, n_used, q_max, max_iter):
    """The rule of ``cluster`` for one sounding, in numpy: D [n, n] symmetric with a zero diagonal, only the first ``n_used`` models
    count (clamped to 0 .. n).  Returns {medoid int32 [q_max, q_max], label int32 [q_max, n], nearest, second f64 [q_max, n], iterations
    int32 [q_max], converged uint8 [q_max], n_found}.

    With m = n_used: if m == 0 or an entry of D[:m, :m] is non-finite or negative, n_found = 0 and every stage is not found.  Every sum
    below runs over j = 0 .. m - 1 in ascending order in fp64, every argmin / argmax takes the lowest index among equals.
    Stage 1: the medoid is argmin_i sum_j D[j, i].  Stage q > 1: stage q - 1's final medoids plus the candidate c with the greatest gain
    g[c] = sum_j max(nearest[j] - D[j, c], 0) against stage q - 1's final assignment; if that gain is 0.0 there are fewer than q distinct
    models: this stage and the later ones are not found and n_found = q - 1.  Then, at most ``max_iter`` times: assign every model j to
    the medoid c_p with the least D[c_p, j] (ties to the medoid that joined first; ``nearest`` and ``second`` are the least and the
    second-least of those entries, second NaN at stage 1); per family the new medoid is the member i with the least sum_{j in the family}
    D[j, i] (a family without a member keeps its medoid); if no medoid changed, converged = 1 and the stage ends.  When the cap is
    reached the models are assigned once more to the current medoids and converged = 0.  ``iterations`` counts the updates.  A stage not
    found: medoid -1, label -1, nearest and second NaN, iterations 0, converged 0; label -1 and NaN for the models j >= m of every stage."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError("families_reference: D [n, n]")
    n = D.shape[0]
    Q, max_iter = check_int(q_max, 1, MAX_FAMILIES, "q_max"), check_int(max_iter, 0, 2 ** 31 - 1, "max_iter")
    out = dict(medoid=np.full((Q, Q), -1, dtype=np.int32), label=np.full((Q, n), -1, dtype=np.int32), nearest=np.full((Q, n), np.nan),
               second=np.full((Q, n), np.nan), iterations=np.zeros(Q, dtype=np.int32), converged=np.zeros(Q, dtype=np.uint8), n_found=np.int32(0))
    m = min(max(int(n_used), 0), n)
    P = D[:m, :m]
    if m == 0 or not np.all(np.isfinite(P) & (P >= 0.0)):
        return out
    column_sum = lambda terms: np.cumsum(terms, axis=0)[-1]      # noqa: E731  (cumsum: row after row, the order of the rule)
    med, near = [], None
    for q in range(1, Q + 1):
        if q == 1:
            med = [int(np.argmin(column_sum(P)))]
        else:
            gain = column_sum(np.maximum(near[:, None] - P, 0.0))
            c = int(np.argmax(gain))
            if gain[c] == 0.0:
                break
            med = med + [c]
        it, conv = 0, 0
        while True:
            to_medoid = P[med, :]                                # [q, m]: the medoids' rows
            lab = np.argmin(to_medoid, axis=0)
            ordered = np.sort(to_medoid, axis=0)
            near, sec = ordered[0], (ordered[1] if q > 1 else np.full(m, np.nan))
            if it >= max_iter:
                break
            it += 1
            new = list(med)
            for p in range(q):
                member = lab == p
                if member.any():
                    idx = np.flatnonzero(member)
                    new[p] = int(idx[np.argmin(column_sum(np.where(member[:, None], P[:, idx], 0.0)))])      # (the members' columns only)
            if new == med:
                conv = 1
                break
            med = new
        st = q - 1
        out["medoid"][st, :q] = med
        out["label"][st, :m], out["nearest"][st, :m], out["second"][st, :m] = lab, near, sec
        out["iterations"][st], out["converged"][st] = it, conv
        out["n_found"] = np.int32(q)
    return out


# ---- which models --------------------------------------------------------------------------------------------------------------------

def used_rows(ens, chains=1, max_models=1024):
    """The models the families are made of: the filled slots of the chains ``ensembles.segments`` uses (chains with >= 8 filled slots,
    the same 2 N slots of each: what the diagnostics and the correlation use), chain after chain, thinned at the regular stride
    ceil(n / max_models) and compacted to a prefix.  ``ens.k`` [B, n_slots] (torch on any device, or numpy), ``chains`` = C chains on
    the slot axis.  Returns (rows int32 [B, n_max], n_used int32 [B], chain_of int32 [B, n_max]) -- -1 past a sounding's n_used -- as
    torch tensors on the device of ``ens.k`` (numpy for a numpy ``ens.k``); n_max = max(1, max n_used)."""
    k = ens.k
    tensor = torch.is_tensor(k)
    kn = k.cpu().numpy() if tensor else np.asarray(k)
    if kn.ndim != 2 or kn.shape[1] < 1 or kn.dtype.kind not in "iu":
        raise ValueError("used_rows: k is an integer array [B, n_slots]")
    C = check_chains(chains, kn.shape[1])
    max_models = check_int(max_models, 1, MAX_MODELS, "max_models")
    B, per = kn.shape[0], kn.shape[1] // C
    count = (kn.reshape(B, C, per) > 0).sum(axis=2)
    start, seg_m, seg_n, _ = segments(count, per)
    lists = []
    for b in range(B):
        first = start[b, 0:seg_m[b]:2].astype(np.int64)             # the used chains' first slots
        every = (first[:, None] + np.arange(2 * int(seg_n[b]))[None, :]).reshape(-1)
        lists.append(every[::max(1, -(-every.size // max_models))])
    n_used = np.array([r.size for r in lists], dtype=np.int32)
    n_max = max(1, int(n_used.max(initial=0)))
    rows = np.full((B, n_max), -1, dtype=np.int32)
    for b, r in enumerate(lists):
        rows[b, :r.size] = r
    chain_of = np.where(rows >= 0, rows // per, -1).astype(np.int32)
    if tensor:
        return tuple(torch.as_tensor(a).to(k.device) for a in (rows, n_used, chain_of))
    return rows, n_used, chain_of


# ---- the entries ---------------------------------------------------------------------------------------------------------------------

def distance(ens, rows, z0, z1, measure="linear", squared=False, block=None, log10=True):
    """D f64 [B, n, n] on the device: the distance (``distance_reference`` states the rule; ``squared``: D^2) between the models
    ``rows`` int32 [B, n] (slot indices; a row outside the slots or an empty slot is absent: NaN) of every sounding of the ensemble over
    the window [z0, z1] with ``measure`` "linear" or "log".  ``log10=False``: the stored values as they are.  ``block``: soundings per
    launch (None: as many as keep a launch's output under 2 GiB).  One kernel (gbp_ensemble_distance)."""
    entry = "gbp_ensemble_distance"
    are_tensors((ens.k, ens.edges, ens.sigma, rows), "families", "distance", entry)
    k, edges, sigma, B, ns, K = check_ensemble(ens, rows=rows, what="distance", max_rows=MAX_MODELS)
    if ns < 1 or not 1 <= K <= MAX_K:
        raise ValueError("ensemble: at least one slot and K in [1, %d]" % MAX_K)
    z0, z1, log = check_window(z0, z1, measure)
    check_block(block, "distance")
    on_device((k, edges, sigma, rows), "families", "distance", entry)
    rows, dev = rows.contiguous(), k.device
    n = rows.shape[1]
    out = torch.empty((B, n, n), dtype=torch.float64, device=dev)
    if B > 0:
        tiles = (n + 15) // 16
        most = (2 ** 32 - 1) // (256 * (tiles * (tiles + 1) // 2))         # soundings one launch can take: 256 threads per tile pair
        step = min(max(1, DISTANCE_BLOCK_BYTES // (n * n * 8)), most) if block is None else int(block)
        for b0 in range(0, B, step):
            s = slice(b0, min(B, b0 + step))
            _lib.call(entry, dev, s.stop - s.start, ns, K, k[s], edges[s], sigma[s], n, rows[s], z0, z1, log, int(bool(log10)), int(bool(squared)),
                      out[s])
    return out


def summaries(stages):
    """cost, silhouette [B, Q] and share [B, Q, Q] of the stages {label [B, Q, n], nearest, second [B, Q, n], n_found [B]} (torch, any
    device): cost = sum of nearest over the used models; silhouette = the mean over the used models of (second - nearest) / second with
    0 / 0 counting 0 -- the medoid-based, simplified silhouette; NaN at stage 1 --; share[b, q - 1, p] = the fraction of the used models
    in family p (0 for p >= q).  All three are NaN for a stage not found."""
    label, nearest, second, n_found = stages["label"], stages["nearest"], stages["second"], stages["n_found"]
    B, Q, n = label.shape
    used = label >= 0
    count = used.sum(dim=2).to(torch.float64)
    found = torch.arange(1, Q + 1, device=label.device)[None, :] <= n_found[:, None]
    nan = torch.full((), float("nan"), dtype=torch.float64, device=label.device)
    zero = torch.zeros((), dtype=torch.float64, device=label.device)
    cost = torch.where(found, torch.where(used, nearest, zero).sum(dim=2), nan)
    width = torch.where(used & (second > 0), (second - nearest) / second, zero)
    silhouette = torch.where(found, width.sum(dim=2) / count, nan)
    silhouette[:, 0] = nan
    members = (label[:, :, None, :] == torch.arange(Q, device=label.device)[None, None, :, None]).sum(dim=3).to(torch.float64)
    share = torch.where(found[:, :, None], members / count[:, :, None], nan)
    return cost, silhouette, share


def cluster(dist, n_used, max_families=4, max_iter=100):
    """k-medoids on ``dist`` f64 [B, n, n] (symmetric, zero diagonal: what ``distance`` gives) for 1 .. ``max_families`` families, on the
    first ``n_used`` int32 [B] models of every sounding (``families_reference`` states the rule).  Returns {medoid int32 [B, Q, Q], label
    int32 [B, Q, n], nearest, second f64 [B, Q, n], iterations int32 [B, Q], converged bool [B, Q], n_found int32 [B]} from one kernel
    (gbp_distance_families), and cost, silhouette f64 [B, Q], share f64 [B, Q, Q] (``summaries``)."""
    are_tensors((dist, n_used), "families", "cluster", "gbp_distance_families")
    if dist.ndim != 3 or dist.shape[1] != dist.shape[2] or not 1 <= dist.shape[1] <= MAX_MODELS or n_used.shape != (dist.shape[0],):
        raise ValueError("cluster: dist [B, n, n] with 1 <= n <= %d and n_used [B]" % MAX_MODELS)
    if dist.dtype != torch.float64 or n_used.dtype != torch.int32:
        raise TypeError("cluster: dist is float64 and n_used is int32")
    Q, max_iter = check_int(max_families, 1, MAX_FAMILIES, "max_families"), check_int(max_iter, 0, 2 ** 31 - 1, "max_iter")
    on_device((dist, n_used), "families", "cluster", "gbp_distance_families")
    dist, n_used, dev = dist.contiguous(), n_used.contiguous(), dist.device
    B, n = dist.shape[0], dist.shape[1]
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)       # noqa: E731  (the kernel writes every entry)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)     # noqa: E731
    out = dict(medoid=i32(B, Q, Q), label=i32(B, Q, n), nearest=f64(B, Q, n), second=f64(B, Q, n), iterations=i32(B, Q), n_found=i32(B))
    conv = torch.empty((B, Q), dtype=torch.uint8, device=dev)
    if B > 0:
        _lib.call("gbp_distance_families", dev, B, n, dist, n_used, Q, max_iter, out["medoid"], out["label"], out["nearest"], out["second"],
                  out["iterations"], conv, out["n_found"])
    out["converged"] = conv.bool()
    out["cost"], out["silhouette"], out["share"] = summaries(out)
    return out


def select(stages, min_silhouette=0.7, min_share=0.05):
    """n_families int32 [B]: the found stage q >= 2 with the greatest silhouette (the fewest families among equals) among those whose
    smallest family holds at least ``min_share`` of the used models and whose silhouette is at least ``min_silhouette``; 1 when no stage
    passes, 0 when no stage was found at all.  ``stages``: what ``cluster`` returns (silhouette, share, n_found; torch on any device, or
    numpy: then numpy is returned).  0.7 is Kaufman and Rousseeuw's "strong structure" convention -- a documented default, not a fitted
    number: a unimodal posterior typically reads 0.4 - 0.5 at two families."""
    for v, what in ((min_silhouette, "min_silhouette"), (min_share, "min_share")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError("%s must be a number in [0, 1]" % what)
    numpy = not torch.is_tensor(stages["silhouette"])
    sil, share, n_found = (torch.as_tensor(stages[n]) for n in ("silhouette", "share", "n_found"))
    B, Q = sil.shape
    q = torch.arange(1, Q + 1, device=sil.device)
    inside = q[None, :, None] >= q[None, None, :]                      # family p < q of stage q
    smallest = torch.where(inside, share, torch.ones((), dtype=share.dtype, device=sil.device)).min(dim=2).values
    ok = (q[None, :] >= 2) & (q[None, :] <= n_found[:, None]) & (sil >= float(min_silhouette)) & (smallest >= float(min_share))
    score = torch.where(ok, sil, torch.full((), -1.0, dtype=sil.dtype, device=sil.device))
    best = score.argmax(dim=1)                                         # (the first of equals: the fewest families)
    nf = torch.where(ok.any(dim=1), best + 1, torch.ones_like(best))
    nf = torch.where(n_found > 0, nf, torch.zeros_like(nf)).to(torch.int32)
    return nf.numpy() if numpy else nf


def families(ens, z1, z0=0.0, measure="linear", chains=1, max_families=4, max_models=1024, max_iter=100, min_silhouette=0.7, min_share=0.05,
             keep_distance=False, block=None):
    """The representative model and the families of the kept models of every sounding over the window [z0, z1] (``used_rows``,
    ``distance``, ``cluster`` and ``select`` in turn; ``chains`` = C chains on the slot axis, as ``replicates.Pooled`` yields them).
    Returns what ``cluster`` returns and rows, n_used, chain_of (``used_rows``), n_families int32 [B] (``select``), and

    central_row int32 [B], central_k int32 [B], central_edges / central_sigma f64 [B, K], central_mean_distance f64 [B]: the stage-1
        medoid -- the kept model with the least mean distance to all used models -- its slot, the model, and that mean distance
        (-1, 0, NaN where no stage was found);
    family_share f64 [B, Q], family_row int32 [B, Q], family_k int32 [B, Q], family_edges / family_sigma f64 [B, Q, K]: the families of
        the selected stage ordered by share, largest first (the family that joined first among equals), and their medoid models; 0, -1,
        0, NaN beyond n_families;
    family_label int32 [B, n_max]: the family of every used model in that order (-1 past n_used);
    family_chain_share f64 [B, Q, C]: the share of each chain's used models in each family (NaN for a chain that is not used).

    ``keep_distance``: also ``distance`` f64 [B, n_max, n_max].  The medoid models are gathered with torch indexing."""
    z0, z1, _ = check_window(z0, z1, measure)
    Q = check_int(max_families, 1, MAX_FAMILIES, "max_families")
    check_block(block, "families")
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    are_tensors((k, edges, sigma), "families", "families", "gbp_ensemble_distance")
    if k.ndim != 2:
        raise ValueError("ensemble: k [B, n_slots], edges and sigma [B, n_slots, K]")
    C = check_chains(chains, k.shape[1])
    rows, n_used, chain_of = used_rows(ens, chains=C, max_models=max_models)
    D = distance(ens, rows, z0, z1, measure=measure, block=block)
    out = cluster(D, n_used, max_families=Q, max_iter=max_iter)
    nf = select(out, min_silhouette=min_silhouette, min_share=min_share)
    B, n, K, dev = rows.shape[0], rows.shape[1], edges.shape[2], k.device
    out.update(rows=rows, n_used=n_used, chain_of=chain_of, n_families=nf)
    if keep_distance:
        out["distance"] = D
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    batch = torch.arange(B, device=dev)

    def models(index, present):
        """Slot, k, edges, sigma of the models ``index`` [B, ...] of the lists (``present``: where there is one)."""
        slot = torch.gather(rows.long(), 1, index.clamp(min=0).reshape(B, index.shape[1:].numel())).reshape(index.shape).clamp(min=0)
        at = (batch.reshape((B,) + (1,) * (index.ndim - 1)), slot)
        return (torch.where(present, slot, torch.full_like(slot, -1)).to(torch.int32), torch.where(present, k[at], torch.zeros_like(k[at])),
                torch.where(present[..., None], edges[at], nan), torch.where(present[..., None], sigma[at], nan))

    found = out["n_found"] > 0
    out["central_row"], out["central_k"], out["central_edges"], out["central_sigma"] = models(out["medoid"][:, 0, 0].long(), found)
    out["central_mean_distance"] = out["cost"][:, 0] / n_used.to(torch.float64)
    stage = (nf.long() - 1).clamp(min=0)                               # the selected stage
    q = torch.arange(Q, device=dev)
    inside = (q[None, :] < nf[:, None])                                # [B, Q]
    share = torch.where(inside, out["share"][batch, stage], torch.full((), -1.0, dtype=torch.float64, device=dev))
    order = torch.argsort(share, dim=1, descending=True, stable=True)  # position in the output -> the family's position in the stage
    out["family_share"] = torch.where(inside, torch.gather(share, 1, order), torch.zeros((), dtype=torch.float64, device=dev))
    out["family_row"], out["family_k"], out["family_edges"], out["family_sigma"] = models(torch.gather(out["medoid"][batch, stage].long(), 1, order), inside)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, q[None, :].expand(B, Q).contiguous())      # the family's position in the stage -> its position in the output
    lab = out["label"][batch, stage].long()
    fl = torch.where(lab >= 0, torch.gather(rank, 1, lab.clamp(min=0)), torch.full_like(lab, -1))
    fl = torch.where((nf > 0)[:, None], fl, torch.full_like(fl, -1))
    out["family_label"] = fl.to(torch.int32)
    c = torch.arange(C, device=dev)
    in_chain = chain_of[:, None, :] == c[None, :, None]               # [B, C, n]
    in_family = fl[:, :, None] == q[None, None, :]                     # [B, n, Q]
    both = (in_chain[:, :, :, None] & in_family[:, None, :, :]).sum(dim=2).to(torch.float64)         # [B, C, Q]
    per_chain = in_chain.sum(dim=2).to(torch.float64)
    out["family_chain_share"] = torch.where(per_chain[:, :, None] > 0, both / per_chain[:, :, None], nan).transpose(1, 2).contiguous()
    return out


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def _parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m geobipy_amd.families",
                                description="The representative model and the families of the kept models of a saved ensemble; writes <name>.families.npz")
    p.add_argument("ensemble", help="an ensemble written by ensembles.save (.npz)")
    p.add_argument("--depth", type=float, required=True, metavar="Z1", help="the bottom of the depth window (m)")
    p.add_argument("--from", dest="z0", type=float, default=0.0, metavar="Z0", help="the top of the depth window (default 0)")
    p.add_argument("--measure", choices=MEASURES, default="linear", help="weigh depth linearly or by its logarithm (log needs --from > 0)")
    p.add_argument("--chains", type=int, default=1, help="replicate chains on the slot axis (default 1)")
    p.add_argument("--max-families", type=int, default=4, metavar="Q", help="the most families to look for, 1 .. 8 (default 4)")
    p.add_argument("--max-models", type=int, default=1024, metavar="N", help="the most models per sounding, 1 .. 4096 (default 1024)")
    p.add_argument("--device", default="cuda:0")
    return p


def parse_args(argv=None):
    """The command line of ``python -m geobipy_amd.families`` as (path, keywords of ``families``, device); refuses before any device work."""
    p = _parser()
    a = p.parse_args(argv)
    try:
        check_window(a.z0, a.depth, a.measure)
        check_int(a.chains, 1, 8, "--chains")
        check_int(a.max_families, 1, MAX_FAMILIES, "--max-families")
        check_int(a.max_models, 1, MAX_MODELS, "--max-models")
    except ValueError as e:
        p.error(str(e))
    return a.ensemble, dict(z1=a.depth, z0=a.z0, measure=a.measure, chains=a.chains, max_families=a.max_families, max_models=a.max_models), a.device


def families_path(path):
    """<name>.families.npz beside the ensemble <name>.npz."""
    return (path[:-4] if path.endswith(".npz") else path) + ".families.npz"


def main(argv=None):
    from .ensembles import load
    path, kw, device = parse_args(argv)
    ens = load(path, device=device)
    d = families(ens, **kw)
    out = families_path(path)
    np.savez_compressed(out, z0=kw["z0"], z1=kw["z1"], measure=kw["measure"], thin=ens.thin, **{n: v.cpu().numpy() for n, v in d.items()})
    print("wrote", out)
    return out


if __name__ == "__main__":
    main()
