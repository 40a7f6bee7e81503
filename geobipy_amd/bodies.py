"""Connected bodies of joint realisations (csrc/gbp_bodies.h k_bodies_label through gbp_bodies_label): what
``sections.draw`` and ``sections.graph_draw`` are drawn for -- whether a unit is continuous from A to B, how large the largest
conductor is, whether it carries on from one line to the next.

The rule.  Nodes are the cells (s, c) of a realisation's raster [S, C] (depth, or ONE elevation axis: ``elevation.resample`` first on
terrain, so that lateral adjacency is horizontal).  A cell is a member iff lo <= v <= hi in fp64: a NaN never is, +-inf bounds give
one-sided thresholds.  (s, c) - (s, c + 1) are adjacent, and (u, c) - (v, c) for every edge (eu[e], ev[e]) of the survey graph
(undirected, either direction, repeats allowed).  A body is a connected set of members.  Per realisation, all integers: ``label``
int32, -1 for a non-member and otherwise the smallest linear index s * C + c of the cell's body; ``cells`` int32, at a body's root (the
cell whose index is its label) the number of its cells, 0 elsewhere; ``measure_q`` int64, at the root the sum of q(s, c) =
rint((a[s] * t[c]) / unit) with unit = (max a * max t) * 2^-30, 0 elsewhere: every q <= 2^30, fewer than 2^31 cells, so the sum is exact
and order-free -- the one step from floating point (the precedent is ``ensembles.quantise_weights``).  measure = measure_q * unit.
``label_reference`` states the rule in numpy with its own loops; the device is held to it with ==."""
import numpy as np
import torch

from . import _lib
from ._args import are_tensors, check_block, check_int, check_ptr, host, on_device

MAX_COLUMNS = 4096
MAX_REALISATIONS = 65536
MAX_CELLS = 2 ** 31 - 1
CELL_BYTES = 16
Q_BITS = 30


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def member_reference(raster, lo, hi):
    """bool, the raster's shape: lo <= v <= hi (a NaN is never a member)."""
    v = np.asarray(raster, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= np.float64(lo)) & (v <= np.float64(hi))


def _check_bounds(lo, hi, what):
    for v, name in ((lo, "lo"), (hi, "hi")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError("%s: %s must be a number, not NaN (-inf / inf: no bound)" % (what, name))
    return float(lo), float(hi)


def _check_edges(eu, ev, S, what):
    eu, ev = np.asarray(host(eu)).reshape(-1), np.asarray(host(ev)).reshape(-1)
    if eu.size != ev.size:
        raise ValueError("%s: eu and ev must hold one entry per edge" % what)
    if eu.size and (eu.dtype.kind not in "iu" or ev.dtype.kind not in "iu"):
        raise TypeError("%s: eu and ev are integers" % what)
    eu, ev = eu.astype(np.int64), ev.astype(np.int64)
    if eu.size >= 2 ** 30:
        raise ValueError("%s: at most 2^30 - 1 edges" % what)
    if eu.size and (min(eu.min(), ev.min()) < 0 or max(eu.max(), ev.max()) >= S):
        raise ValueError("%s: an edge's sounding lies outside 0 .. S - 1 (S = %d)" % (what, S))
    return eu, ev


def measure_unit(a, t, what="bodies.measure_unit"):
    """(a, t, unit): ``a`` [S] and ``t`` [C] as float64, finite and >= 0, and unit = (max a * max t) * 2^-30; unit == 0 is refused."""
    a, t = np.asarray(host(a), dtype=np.float64).reshape(-1), np.asarray(host(t), dtype=np.float64).reshape(-1)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(t)) and np.all(a >= 0.0) and np.all(t >= 0.0)):
        raise ValueError("%s: a and t must be finite and >= 0" % what)
    unit = float((a.max(initial=0.0) * t.max(initial=0.0)) * 2.0 ** -Q_BITS)
    if not (unit > 0.0 and np.isfinite(unit)):
        raise ValueError("%s: unit = (max a * max t) * 2^-30 must be finite and > 0 (a measure of zero everywhere has no bodies to size)" % what)
    return a, t, unit


def quantise(a, t, what="bodies.quantise"):
    """(q int64 [S, C], unit): q(s, c) = rint((a[s] * t[c]) / unit), one IEEE operation each."""
    a, t, unit = measure_unit(a, t, what)
    return np.rint((a[:, None] * t[None, :]) / unit).astype(np.int64), unit


def label_reference(member, eu, ev, a=None, t=None):
    """The rule, in numpy with its own loops (a union-find whose root is the smallest index).  ``member`` bool [S, C] or [R, S, C];
    ``eu`` / ``ev`` [E]; ``a`` [S], ``t`` [C]: with both, ``measure_q`` and ``unit``.  Returns ``label`` int32, ``cells`` int32 (and
    ``measure_q`` int64, ``measure`` f64, ``unit``) in the shape of ``member``."""
    m = np.asarray(member, dtype=bool)
    if m.ndim not in (2, 3):
        raise ValueError("bodies.label_reference: member is [S, C] or [R, S, C]")
    m3 = m.reshape((-1,) + m.shape[-2:])
    R, S, C = m3.shape
    eu, ev = _check_edges(eu, ev, S, "bodies.label_reference")
    if (a is None) != (t is None):
        raise ValueError("bodies.label_reference: a and t are given together or not at all")
    q, unit = (None, None) if a is None else quantise(a, t, "bodies.label_reference")
    if q is not None and q.shape != (S, C):
        raise ValueError("bodies.label_reference: a holds one entry per sounding, t one per column")
    label = np.full((R, S * C), -1, dtype=np.int32)
    cells = np.zeros((R, S * C), dtype=np.int32)
    mq = np.zeros((R, S * C), dtype=np.int64)
    pairs = [(int(u), int(v)) for u, v in zip(eu, ev) if u != v]
    for r in range(R):
        flat = m3[r].reshape(-1)
        parent = list(range(S * C))

        def find(i):
            root = i
            while parent[root] != root:
                root = parent[root]
            while parent[i] != root:
                parent[i], i = root, parent[i]
            return root

        def union(i, j):
            i, j = find(i), find(j)
            if i != j:
                parent[max(i, j)] = min(i, j)

        on = np.flatnonzero(flat)
        for i in on:
            i = int(i)
            if i % C and flat[i - 1]:
                union(i - 1, i)
        for u, v in pairs:
            for c in np.flatnonzero(m3[r, u] & m3[r, v]):
                union(u * C + int(c), v * C + int(c))
        for i in on:
            i = int(i)
            root = find(i)
            label[r, i] = root
            cells[r, root] += 1
            if q is not None:
                mq[r, root] += int(q.reshape(-1)[i])
    out = dict(label=label.reshape(m.shape), cells=cells.reshape(m.shape))
    if q is not None:
        out.update(measure_q=mq.reshape(m.shape), measure=mq.reshape(m.shape).astype(np.float64) * unit, unit=unit)
    return out


# ---- groups -----------------------------------------------------------------------------------------------------------------------------

def sounding_pieces(eu, ev, S):
    """int64 [S]: the smallest sounding of every sounding's connected piece of the graph."""
    parent = np.arange(S, dtype=np.int64)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for u, v in zip(eu, ev):
        u, v = find(int(u)), find(int(v))
        if u != v:
            parent[max(u, v)] = min(u, v)
    return np.array([find(s) for s in range(S)], dtype=np.int64)


def default_groups(eu, ev, S):
    """group_ptr int64 [G + 1]: the connected pieces of the sounding graph in sounding order when every piece is a contiguous range of
    soundings, otherwise one group (none for S == 0)."""
    if S == 0:
        return np.zeros(1, dtype=np.int64)
    piece = sounding_pieces(eu, ev, S)
    at = np.arange(S)
    if np.all((piece[1:] == piece[:-1]) | (piece[1:] == at[1:])):
        return np.concatenate([np.flatnonzero(piece == at), [S]]).astype(np.int64)
    return np.array([0, S], dtype=np.int64)


def check_groups(group_ptr, eu, ev, S, what="bodies.label"):
    """``group_ptr`` as int64 [G + 1] (contiguous ranges, possibly empty) and the group of every edge: no edge may join two."""
    p = check_ptr(group_ptr, S, what, empty=True)
    if p.size - 1 > max(S, 0):
        raise ValueError("%s: more groups than soundings" % what)
    gu = np.searchsorted(p, eu, side="right") - 1                              # p[gu] <= eu < p[gu + 1]: empty groups are passed over
    if eu.size and np.any((ev < p[gu]) | (ev >= p[gu + 1])):
        raise ValueError("%s: an edge joins two groups" % what)
    return p, gu


# ---- the device -------------------------------------------------------------------------------------------------------------------------

def label(raster, lo, hi, eu, ev, group_ptr=None, a=None, t=None, block=None, budget_bytes=4 << 30):
    """The bodies of every realisation of ``raster`` f64 [R, S, C] on the device (the module's docstring states the rule; ``eu`` /
    ``ev`` [E] host integers: ``edge_u`` / ``edge_v`` of ``sections.spatial`` / ``neighbours``, or the consecutive pairs of a line).
    ``group_ptr`` [G + 1] (host): contiguous ranges of soundings that no edge leaves, one workgroup per (realisation, group); None:
    ``default_groups``.  ``a`` [S] and ``t`` [C] (host, finite, >= 0; both or neither): the measure a sounding stands for (a width in m
    for a section, an area in m^2 for a survey: ``sounding_areas``) and the cells' thickness.  Realisations are cut into blocks of
    ``block`` (None: what keeps a call's outputs, 16 B per cell, under ``budget_bytes`` and its cells under 2^31); a realisation's
    outputs do not depend on the cut.

    Returns on the device ``label`` int32, ``cells`` int32 [R, S, C], ``sweeps`` int32 [R, G], and with ``a`` and ``t`` ``measure_q``
    int64 and ``measure`` f64 [R, S, C] (at the roots) and ``unit`` (a float); ``group_ptr`` int64 [G + 1] (numpy)."""
    are_tensors((raster,), "bodies", "label", "gbp_bodies_label")
    if raster.ndim != 3 or raster.shape[0] < 1 or raster.shape[2] < 1:
        raise ValueError("bodies.label: raster is [R, S, C] with R >= 1 and C >= 1")
    R, S, C = (int(v) for v in raster.shape)
    if R > MAX_REALISATIONS or C > MAX_COLUMNS or S * C > MAX_CELLS:
        raise ValueError("bodies.label: at most %d realisations, %d columns and 2^31 - 1 cells a realisation" % (MAX_REALISATIONS, MAX_COLUMNS))
    if raster.dtype != torch.float64:
        raise TypeError("bodies.label: raster is float64")
    lo, hi = _check_bounds(lo, hi, "bodies.label")
    eu, ev = _check_edges(eu, ev, S, "bodies.label")
    if (a is None) != (t is None):
        raise ValueError("bodies.label: a and t are given together or not at all")
    unit = None
    if a is not None:
        if np.size(host(a)) != S or np.size(host(t)) != C:
            raise ValueError("bodies.label: a holds one entry per sounding (%d), t one per column (%d)" % (S, C))
        a, t, unit = measure_unit(a, t, "bodies.label")
    p, gu = check_groups(default_groups(eu, ev, S) if group_ptr is None else group_ptr, eu, ev, S)
    G = p.size - 1
    check_block(block, "bodies.label")
    budget_bytes = check_int(budget_bytes, 1, 2 ** 62, "budget_bytes")
    per = max(S * C, 1)
    if block is None:
        block = max(1, min(budget_bytes // (CELL_BYTES * per), MAX_CELLS // per))
    block = int(min(block, R))
    if block * per > MAX_CELLS or block * max(G, 1) > MAX_CELLS:
        raise ValueError("bodies.label: a block of %d realisations holds 2^31 cells or workgroups or more; lower block" % block)
    on_device((raster,), "bodies", "label", "gbp_bodies_label")
    dev = raster.device
    order = np.argsort(gu, kind="stable")                                      # the entry takes the edges group by group
    t_eu, t_ev = (torch.as_tensor(v[order].astype(np.int32)).to(dev) for v in (eu, ev))
    t_p = torch.as_tensor(p).to(dev)
    t_a, t_t = (None, None) if a is None else (torch.as_tensor(a).to(dev), torch.as_tensor(t).to(dev))
    v = raster.contiguous()
    out = dict(label=torch.empty((R, S, C), dtype=torch.int32, device=dev), cells=torch.empty((R, S, C), dtype=torch.int32, device=dev),
               sweeps=torch.zeros((R, G), dtype=torch.int32, device=dev))
    mq = torch.empty((R, S, C), dtype=torch.int64, device=dev) if a is not None else None
    for r0 in range(0, R, block):
        r1 = min(r0 + block, R)
        _lib.call("gbp_bodies_label", dev, r1 - r0, S, C, eu.size, G, t_p, t_eu if eu.size else None, t_ev if eu.size else None, v[r0:r1], lo, hi,
                  t_a, t_t, 0.0 if unit is None else unit, out["label"][r0:r1], out["cells"][r0:r1], None if mq is None else mq[r0:r1],
                  out["sweeps"][r0:r1])
    if mq is not None:
        out.update(measure_q=mq, measure=mq.to(torch.float64) * unit, unit=unit)
    out["group_ptr"] = p
    return out


def _cell_groups(lab):
    """int64 [S * C] on the device: the group of every cell."""
    R, S, C = lab["label"].shape
    p = np.asarray(lab["group_ptr"], dtype=np.int64)
    gid = np.repeat(np.arange(p.size - 1, dtype=np.int64), np.diff(p))
    return torch.as_tensor(np.repeat(gid, C)).to(lab["label"].device), p.size - 1


def summary(lab, min_cells=1):
    """Per (realisation, group) of a result of ``label``, over the bodies of at least ``min_cells`` cells, on the device with integer
    decisions only: ``n_bodies`` int64 [R, G]; ``largest_root`` int64 (the linear index of the largest body's root, by ``measure_q``
    -- by ``cells`` without a measure --, ties to the smallest root; -1: no body); ``largest_cells`` int64; and with a measure
    ``largest_measure`` and ``member_measure`` f64 (the sum over the bodies counted)."""
    min_cells = check_int(min_cells, 1, MAX_CELLS, "bodies.summary: min_cells")
    cells = lab["cells"]
    are_tensors((cells, lab["label"]), "bodies", "summary", "gbp_bodies_label")
    R, S, C = cells.shape
    dev = cells.device
    gid, G = _cell_groups(lab)
    has = "measure_q" in lab
    n = cells.reshape(R, S * C).long()
    root = n >= min_cells
    size = lab["measure_q"].reshape(R, S * C) if has else n
    idx = gid[None, :].expand(R, S * C)
    zero = torch.zeros((R, G), dtype=torch.int64, device=dev)
    key = torch.where(root, size, torch.full((), -1, dtype=torch.int64, device=dev))
    best = torch.full((R, G), -1, dtype=torch.int64, device=dev).scatter_reduce_(1, idx, key, "amax", include_self=True) if S * C else zero - 1
    at = torch.arange(S * C, dtype=torch.int64, device=dev)[None, :].expand(R, S * C)
    big = torch.full((), S * C, dtype=torch.int64, device=dev)
    where = torch.where(root & (key == torch.gather(best, 1, idx)), at, big) if S * C else at
    first = torch.full((R, G), S * C, dtype=torch.int64, device=dev).scatter_reduce_(1, idx, where, "amin", include_self=True) if S * C else zero + S * C
    none = first >= S * C
    pick = first.clamp(max=max(S * C - 1, 0))
    out = dict(n_bodies=zero.clone().scatter_add_(1, idx, root.long()) if S * C else zero,
               largest_root=torch.where(none, zero - 1, first),
               largest_cells=torch.where(none, zero, torch.gather(n, 1, pick)) if S * C else zero)
    if has:
        q = torch.where(root, size, torch.zeros((), dtype=torch.int64, device=dev))
        total = zero.clone().scatter_add_(1, idx, q) if S * C else zero
        out.update(largest_measure=torch.where(none, zero, best).to(torch.float64) * lab["unit"], member_measure=total.to(torch.float64) * lab["unit"])
    return out


def _check_cells(cells, S, C, what):
    c = np.asarray(host(cells))
    if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1 or c.dtype.kind not in "iu":
        raise ValueError("%s: cells are (sounding, column) pairs, integers [Q, 2] with Q >= 1" % what)
    c = c.astype(np.int64)
    if c.min() < 0 or c[:, 0].max() >= S or c[:, 1].max() >= C:
        raise ValueError("%s: a cell lies outside the raster (S = %d, C = %d)" % (what, S, C))
    return c


def connected(lab, a_cell, b_cell):
    """Is the unit continuous from A to B: ``connected`` bool [R, Q], true where both cells are members and carry one label, and
    ``probability`` f64 [Q], its share of the realisations.  ``a_cell`` / ``b_cell``: (sounding, column) pairs [Q, 2] (host)."""
    L = lab["label"]
    are_tensors((L,), "bodies", "connected", "gbp_bodies_label")
    R, S, C = L.shape
    ca, cb = _check_cells(a_cell, S, C, "bodies.connected"), _check_cells(b_cell, S, C, "bodies.connected")
    if ca.shape != cb.shape:
        raise ValueError("bodies.connected: a_cell and b_cell hold one pair per question")
    flat = L.reshape(R, S * C)
    la, lb = (flat[:, torch.as_tensor(c[:, 0] * C + c[:, 1]).to(L.device)] for c in (ca, cb))
    one = (la >= 0) & (la == lb)
    return dict(connected=one, probability=one.to(torch.float64).mean(dim=0))


def reach(lab, seeds):
    """The connection probability map of a borehole screen: for every seed cell (sounding, column) of ``seeds`` [Q, 2] (host) ``share``
    f64 [Q, S, C], the share of realisations in which the cell belongs to the seed's body; ``seed_member`` f64 [Q], the share in which
    the seed is a member at all; ``cells`` int64 [R, Q], the size of the seed's body (0 where the seed is not a member) and, with a
    measure, ``measure`` f64 [R, Q]."""
    L = lab["label"]
    are_tensors((L,), "bodies", "reach", "gbp_bodies_label")
    R, S, C = L.shape
    sd = _check_cells(seeds, S, C, "bodies.reach")
    flat = L.reshape(R, S * C)
    ls = flat[:, torch.as_tensor(sd[:, 0] * C + sd[:, 1]).to(L.device)]         # [R, Q]
    member = ls >= 0
    share = torch.stack([((flat == ls[:, q:q + 1]) & member[:, q:q + 1]).to(torch.float64).mean(dim=0) for q in range(sd.shape[0])]).reshape(-1, S, C)
    at = ls.long().clamp(min=0)
    zero = torch.zeros((), dtype=torch.int64, device=L.device)
    out = dict(share=share, seed_member=member.to(torch.float64).mean(dim=0),
               cells=torch.where(member, torch.gather(lab["cells"].reshape(R, S * C).long(), 1, at), zero))
    if "measure_q" in lab:
        out["measure"] = torch.where(member, torch.gather(lab["measure_q"].reshape(R, S * C), 1, at), zero).to(torch.float64) * lab["unit"]
    return out


def sounding_areas(plan):
    """float64 [S] (numpy), m^2: the area a sounding stands for on the grid of a ``gridding.SibsonPlan`` -- the number of pixels whose
    ``plan.index`` is the sounding times dx * dy.  The ``a`` of a survey: with it ``measure`` is a volume, the analogue of
    ``sections.exceedance_area`` across lines."""
    idx = plan.index.reshape(-1).long()
    idx = idx[(idx >= 0) & (idx < plan.n_soundings)]
    count = torch.bincount(idx, minlength=plan.n_soundings).cpu().numpy().astype(np.float64)
    dx, dy = float(plan.x_edges[1] - plan.x_edges[0]), float(plan.y_edges[1] - plan.y_edges[0])
    return count * (dx * dy)
