"""Model families on the device (csrc/gbp_ensemble_families.h k_layered_distance<linear / log> and k_distance_families;
geobipy_amd.families distance / cluster / families).

The distance is held to the rule ``families.distance_reference`` evaluated in long double -- never to device output -- with bounds that
are a priori.  With U = 2^-52, K the layer capacity, D2 the rule's squared distance and a_max the largest |log10 sigma|:
    stored values (log10 = 0)   |dD2| <= (2 K + 16) U D2            (+ 8 U D2 for the log measure: ln of every segment)
    log10 taken on the device   |dD2| <= the same + 16 U a_max D + (8 U a_max)^2
(every term mu d^2 is >= 0 and at most 2 K of them are added, so the first bound holds for any contraction; a device log10 within 4 U
relative -- what test_ensemble_correlation_gpu.py assumes of the same expression -- moves a difference d by at most 8 U a_max, and
(d + e)^2 - d^2 = 2 d e + e^2 averages to at most 16 U a_max D + (8 U a_max)^2).  For D = sqrt(D2) with e the bound of D2:
|dD| <= min(e / D, sqrt(e)) + 2 U D (sqrt(x + e) - sqrt(x) = e / (sqrt(x + e) + sqrt(x)), which is below both).  Symmetry, the diagonal,
identical models, NaN patterns and repeated calls are held with ``==``.  Every case prints used / bound.

The clustering is held to ``families.families_reference`` on the same matrix with ``==`` for every output."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import ensembles, families
from test_families import PLANTED, planted, same_partition
from test_rjmcmc_gpu import GOLDEN, _chains

U = 2.0 ** -52


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: v.cpu().numpy() for n, v in d.items() if torch.is_tensor(v)}


def _to_device(k, edges, sigma):
    dev = _dev()
    k, edges, sigma = (torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (k, edges, sigma))
    return ensembles.Ensemble(k, edges, sigma, torch.ones(k.shape, dtype=torch.float64, device=dev), (k > 0).sum(dim=1), 1,
                              torch.zeros(k.shape[0], dtype=torch.float64, device=dev))


def _hand_made(n, K, seed):
    """B = 2 soundings, n_slots = n + 3 slots and a list of n rows each.  Slots: random k in 1 .. K (a half-space, a full model among
    them), interfaces in and around the window 5 .. 200 m -- some exactly at its ends, some shared with the slot before --, slot 1 a copy
    of slot 0 and slot n + 2 empty.  Rows: a shuffle of the slots that, where n allows, names the empty slot, the copy, -1, a slot past
    the end, and one slot twice."""
    rng = np.random.default_rng(seed)
    B, ns = 2, n + 3
    k = np.zeros((B, ns), dtype=np.int32)
    edges, sigma = np.full((B, ns, K), np.inf), np.full((B, ns, K), np.nan)
    for b in range(B):
        for s in range(ns - 1):
            kk = [1, K, min(2, K)][s] if s < 3 else int(rng.integers(1, K + 1))
            e = np.sort(rng.uniform(0.0, 260.0, kk - 1))
            if kk > 1 and s % 3 == 0:
                e[rng.integers(0, kk - 1)] = [5.0, 200.0][s % 2]              # an interface exactly at an end of the window
            if kk > 1 and s > 3 and k[b, s - 1] > 1 and s % 4 == 0:
                e[0] = edges[b, s - 1, 0]                                      # one interface shared with the slot before
            e = np.sort(e)
            k[b, s] = kk
            edges[b, s, :kk - 1] = e
            sigma[b, s, :kk] = 10.0 ** rng.uniform(-4.0, 1.0, kk)
            if kk < K:
                sigma[b, s, kk:] = -1.0                                        # entries past k are never read
        k[b, 1], edges[b, 1], sigma[b, 1] = k[b, 0], edges[b, 0], sigma[b, 0]
    rows = np.stack([rng.permutation(ns)[:n] for _ in range(B)]).astype(np.int32)
    if n >= 15:
        rows[:, 2], rows[:, 5], rows[:, 7], rows[:, 9], rows[:, 11] = ns - 1, -1, ns, 0, 1
        rows[0, 13], rows[1, 13] = rows[0, 12], 2 ** 30
    return k, edges, sigma, rows


def _check_distance(n, K, measure, stored, label):
    z0, z1 = 5.0, 200.0
    k, edges, sigma, rows = _hand_made(n, K, 100 * n + K)
    if stored:                                                                 # the values the rule and the device subtract, as stored
        sigma = np.where(sigma > 0, np.log10(np.where(sigma > 0, sigma, 1.0)), sigma)
    ens, rows_d = _to_device(k, edges, sigma), torch.as_tensor(rows).to(_dev())
    got2 = families.distance(ens, rows_d, z0, z1, measure=measure, squared=True, log10=not stored)
    got1 = families.distance(ens, rows_d, z0, z1, measure=measure, log10=not stored)
    again = families.distance(ens, rows_d, z0, z1, measure=measure, squared=True, log10=not stored)
    assert got2.shape == (2, n, n) and torch.equal(got2.view(torch.int64), again.view(torch.int64))       # a second call, bit for bit
    got2, got1 = got2.cpu().numpy(), got1.cpu().numpy()
    worst2 = worst1 = 0.0
    for b in range(2):
        want2 = families.distance_reference(k[b], edges[b], sigma[b], rows[b], z0, z1, measure=measure, dtype=np.longdouble, stored=stored, squared=True)
        want1 = np.sqrt(want2)
        absent = np.array([not (0 <= r < k.shape[1]) or k[b, min(max(r, 0), k.shape[1] - 1)] <= 0 for r in rows[b]])
        nan = absent[:, None] | absent[None, :]
        for got in (got2[b], got1[b]):
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want2), nan), (label, b)
            assert np.array_equal(got.view(np.int64), got.T.view(np.int64)), (label, b, "symmetry")
            assert np.all(np.diag(got)[~absent] == 0.0), (label, b, "diagonal")
            same = (rows[b][:, None] == rows[b][None, :]) | (np.isin(rows[b], (0, 1))[:, None] & np.isin(rows[b], (0, 1))[None, :])
            assert np.all(got[same & ~nan] == 0.0), (label, b, "identical models")
        ok = ~nan
        if not ok.any():
            continue
        a_max = float(np.nanmax(np.abs(np.log10(np.where(sigma[b] > 0, sigma[b], np.nan))))) if not stored else 0.0
        w2, w1 = want2[ok], want1[ok]
        e2 = (2 * K + 16 + (8 if measure == "log" else 0)) * U * w2 + (16 * U * a_max * w1 + (8 * U * a_max) ** 2 if not stored else 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            e1 = np.minimum(np.where(w1 > 0, e2 / w1, np.inf), np.sqrt(e2)) + 2 * U * w1
        d2, d1 = np.abs(got2[b][ok].astype(np.longdouble) - w2), np.abs(got1[b][ok].astype(np.longdouble) - w1)
        assert np.all(d2 <= e2), (label, b, "D2", float(np.max(d2 - e2)))
        assert np.all(d1 <= e1), (label, b, "D", float(np.max(d1 - e1)))
        live = e2 > 0
        if live.any():
            worst2, worst1 = max(worst2, float(np.max(d2[live] / e2[live]))), max(worst1, float(np.max(d1[live] / e1[live])))
    print("%s used/bound: D2 %.3f D %.3f" % (label, worst2, worst1))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 70])
@pytest.mark.parametrize("K", [1, 2, 7, 64])
def test_distance_against_the_long_double_rule(n, K):
    for measure in ("linear", "log"):
        for stored in (True, False):
            _check_distance(n, K, measure, stored, "n=%d K=%d %s %s" % (n, K, measure, "stored" if stored else "log10"))


def test_distance_of_the_closed_form_pair():
    t1, t2, a, b, z0, z1 = 31.0, 47.5, -2.25, -0.5, 3.0, 120.0
    k = np.array([[2, 2]], dtype=np.int32)
    edges = np.array([[[t1, np.inf, np.inf], [t2, np.inf, np.inf]]])
    sigma = np.array([[[a, b, np.nan], [a, b, np.nan]]])
    rows = torch.tensor([[0, 1]], dtype=torch.int32, device=_dev())
    ens = _to_device(k, edges, sigma)
    for measure, want in (("linear", (t2 - t1) * (a - b) ** 2 / (z1 - z0)), ("log", np.log(t2 / t1) * (a - b) ** 2 / np.log(z1 / z0))):
        D2 = families.distance(ens, rows, z0, z1, measure=measure, squared=True, log10=False).cpu().numpy()[0]
        D = families.distance(ens, rows, z0, z1, measure=measure, log10=False).cpu().numpy()[0]
        print("closed form %s used/bound %.3f" % (measure, abs(D2[0, 1] - want) / (28 * U * want)))
        assert abs(D2[0, 1] - want) <= 28 * U * want and abs(D[0, 1] - np.sqrt(want)) <= 16 * U * np.sqrt(want)
        assert D2[0, 1] == D2[1, 0] and D2[0, 0] == 0.0 and D2[1, 1] == 0.0
    # a narrow, deep window: the measure of the window and of its segments is ln(1 + 1e-5), where ln of a rounded quotient would be
    # wrong by 1e5 U relative; held to the long-double rule within the bound of the stored-value case, (2 K + 24) U D2
    k = np.array([[3, 2]], dtype=np.int32)
    edges = np.array([[[100.0003, 100.0007, np.inf], [100.0005, np.inf, np.inf]]])
    sigma = np.array([[[a, b, -1.0], [b, a, np.nan]]])
    ens = _to_device(k, edges, sigma)
    want = families.distance_reference(k[0], edges[0], sigma[0], [0, 1], 100.0, 100.001, measure="log", dtype=np.longdouble, stored=True, squared=True)
    D2 = families.distance(ens, rows, 100.0, 100.001, measure="log", squared=True, log10=False).cpu().numpy()[0]
    bound = (2 * 3 + 24) * U * want[0, 1]
    print("narrow window log used/bound %.3f" % float(abs(D2[0, 1] - want[0, 1]) / bound))
    assert want[0, 1] > 0 and abs(D2[0, 1] - want[0, 1]) <= bound and D2[0, 1] == D2[1, 0]
    # blocks of soundings give the same bits as one launch
    k, edges, sigma, rows = _hand_made(17, 7, 5)
    ens, rows = _to_device(k, edges, sigma), torch.as_tensor(rows).to(_dev())
    one, two = families.distance(ens, rows, 5.0, 200.0), families.distance(ens, rows, 5.0, 200.0, block=1)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))


# ---- the clustering ------------------------------------------------------------------------------------------------------------------

NAMES = ("medoid", "label", "nearest", "second", "iterations", "converged", "n_found")


def _same_as_the_rule(D, n_used, q_max, max_iter, label):
    """gbp_distance_families on D [B, n, n] (numpy) == families_reference for every output; returns the device's answer."""
    dev = _dev()
    Dd, nu = torch.as_tensor(D).to(dev), torch.as_tensor(np.asarray(n_used, dtype=np.int32)).to(dev)
    got = families.cluster(Dd, nu, max_families=q_max, max_iter=max_iter)
    again = families.cluster(Dd, nu, max_families=q_max, max_iter=max_iter)
    g = _numpy(got)
    for name in g:
        assert np.array_equal(g[name], again[name].cpu().numpy(), equal_nan=True), (label, name, "second call")
    for b in range(D.shape[0]):
        want = families.families_reference(D[b], n_used[b], q_max, max_iter)
        for name in NAMES:
            have = g[name][b]
            ref = np.asarray(want[name])
            if name == "converged":
                ref = ref.astype(bool)
            assert have.dtype == ref.dtype and np.array_equal(have, ref, equal_nan=ref.dtype.kind == "f"), (label, b, name, have, ref)
    return g


def _matrices(n, seed):
    """Five soundings' matrices [5, n, n] and their n_used: integer L1 distances of points on a small grid (ties and identical models), a
    random symmetric integer matrix that is no metric, real distances from the distance kernel on a hand-made ensemble, the degenerate
    matrix of two distinct models, and a matrix with a NaN inside its prefix."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 5, (n, 2)).astype(np.float64)
    grid = np.abs(p[:, None, 0] - p[None, :, 0]) + np.abs(p[:, None, 1] - p[None, :, 1])
    loose = np.triu(rng.integers(0, 4, (n, n)).astype(np.float64), 1)
    loose = loose + loose.T
    k, e, s, _ = planted([20.0, 50.0, 90.0, 120.0, 30.0], seed, n=n)
    e[:, 0] = np.round(e[:, 0])                                                # (interfaces on whole metres: identical models occur)
    s[:, :2] = 10.0 ** np.round(np.log10(s[:, :2]), 1)
    ens = _to_device(k[None], e[None], s[None])
    real = families.distance(ens, torch.arange(n, dtype=torch.int32, device=_dev())[None], 0.0, 150.0).cpu().numpy()[0]
    two = 3.0 * (np.arange(n)[:, None] % 2 != np.arange(n)[None, :] % 2)
    bad = grid.copy()
    bad[n // 2, 0] = bad[0, n // 2] = np.nan
    D = np.stack([grid, loose, real, two, bad])
    n_used = np.array([n, n, n, n, n], dtype=np.int32)
    return D, n_used


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 257, 300])
def test_families_equal_the_host_rule(n):
    D, n_used = _matrices(n, n)
    for q_max, max_iter in ((1, 100), (4, 100), (8, 100), (4, 0), (4, 1)):
        g = _same_as_the_rule(D, n_used, q_max, max_iter, "n=%d q_max=%d max_iter=%d" % (n, q_max, max_iter))
        assert g["n_found"][4] == 0 and np.all(g["medoid"][4] == -1)           # the NaN leaves the other soundings untouched
        assert g["n_found"][3] == min(2, n, q_max) and g["n_found"][0] >= 1
    # n_used differing between the soundings of one launch, 0 and more than n among them
    n_used = np.array([n, max(n // 2, 1), 0, n + 5, max(n // 2, 1)], dtype=np.int32)      # (the NaN sits at n // 2: outside that prefix)
    g = _same_as_the_rule(D, n_used, 4, 100, "n=%d prefixes" % n)
    assert g["n_found"][2] == 0 and np.all(g["label"][2] == -1) and np.all(g["label"][1][:, n_used[1]:] == -1)
    if n >= 4:
        assert g["n_found"][4] >= 1


def test_the_longest_list():
    """n = 4 096, the most both entries take: 256 tile rows (32 896 tile pairs) in the distance, 16 columns per thread and 48 KiB of
    LDS in the clustering.  The distance against the rule on a sample of the rows, the clustering == the rule on the device's matrix."""
    n, K, z0, z1 = 4096, 4, 0.0, 150.0
    k, e, s, which = planted([30.0, 60.0], 7, n=n, K=K)
    ens = _to_device(k[None], e[None], s[None])
    rows = torch.arange(n, dtype=torch.int32, device=_dev())[None]
    D = families.distance(ens, rows, z0, z1)
    pick = np.concatenate([[0, 15, 16, n - 17, n - 16, n - 1], np.random.default_rng(0).choice(n, 40, replace=False)])
    at = torch.as_tensor(pick).to(_dev())
    D2 = families.distance(ens, rows, z0, z1, squared=True)[0][at][:, at].cpu().numpy()
    assert torch.equal(D[0].view(torch.int64), D[0].T.contiguous().view(torch.int64)) and bool(torch.all(torch.diagonal(D[0]) == 0.0))
    want = families.distance_reference(k, e, s, pick, z0, z1, dtype=np.longdouble, squared=True)
    a_max = float(np.abs(np.log10(s[:, :2])).max())
    bound = (2 * K + 16) * U * want + 16 * U * a_max * np.sqrt(want) + (8 * U * a_max) ** 2
    used = np.abs(D2.astype(np.longdouble) - want)
    print("n=4096 used/bound: D2 %.3f" % float(np.max(used / bound)))
    assert np.all(used <= bound)
    host = D.cpu().numpy()
    g = _same_as_the_rule(host, np.array([n], dtype=np.int32), 2, 100, "n=4096")
    assert g["n_found"][0] == 2 and same_partition(g["label"][0, 1], which)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def test_planted_families_on_the_device():
    sets = [planted(tops, 1) for tops in PLANTED]
    k, e, s = (np.stack([q[i] for q in sets]) for i in range(3))
    ens = _to_device(k, e, s)
    d = _numpy(families.families(ens, 150.0, keep_distance=True))
    n = k.shape[1]
    assert d["n_families"].tolist() == [1, 2, 3] and d["n_used"].tolist() == [n] * 3 and np.array_equal(d["rows"], np.tile(np.arange(n), (3, 1)))
    print("silhouettes", np.round(d["silhouette"], 3).tolist())
    for b, (_, _, _, which) in enumerate(sets):
        q = len(PLANTED[b])
        want = families.families_reference(d["distance"][b], n, 4, 100)
        for name in NAMES[:-1]:
            assert np.array_equal(d[name][b], np.asarray(want[name]).astype(d[name].dtype), equal_nan=True), (b, name)
        assert same_partition(d["label"][b, q - 1], which) and same_partition(d["family_label"][b], which)
        assert abs(d["family_share"][b, :q].sum() - 1.0) < 1e-12 and np.all(d["family_share"][b, q:] == 0) and np.all(np.diff(d["family_share"][b, :q]) <= 0)
        for f in range(q):                                                     # a family's medoid is one of its members, and the model is the slot's
            row = d["family_row"][b, f]
            assert d["family_label"][b, row] == f and d["family_k"][b, f] == 2
            assert np.array_equal(d["family_edges"][b, f], e[b, row]) and np.array_equal(d["family_sigma"][b, f], s[b, row], equal_nan=True)
        assert np.all(d["family_row"][b, q:] == -1) and np.all(d["family_k"][b, q:] == 0) and np.isnan(d["family_edges"][b, q:]).all()
        c = d["central_row"][b]
        assert c == d["medoid"][b, 0, 0] and np.array_equal(d["central_edges"][b], e[b, c]) and d["central_k"][b] == 2
        assert d["central_mean_distance"][b] == d["cost"][b, 0] / n and abs(d["central_mean_distance"][b] - d["distance"][b][c].mean()) <= 1e-12
        assert np.allclose(d["family_chain_share"][b, :, 0], d["family_share"][b], rtol=0, atol=1e-15)
    # the sounding with two planted families: the interfaces of the two medoid models sit at the two planted depths
    tops = np.sort(d["family_edges"][1, :2, 0])
    assert abs(tops[0] - 30.0) <= 1.0 and abs(tops[1] - 60.0) <= 1.0


def _consistent(d, ens, C, label):
    """What holds for any ensemble: the central model is a filled slot, the shares sum to 1, labels and nearest agree with the distances."""
    k = ens.k.cpu().numpy()
    B, n = d["rows"].shape
    some = False
    for b in range(B):
        m = int(d["n_used"][b])
        if d["n_found"][b] == 0:
            assert m == 0 and d["central_row"][b] == -1 and d["n_families"][b] == 0, (label, b)
            continue
        some = True
        nf, D = int(d["n_families"][b]), d["distance"][b]
        assert 1 <= nf <= d["n_found"][b] and k[b, d["central_row"][b]] > 0 and d["central_k"][b] == k[b, d["central_row"][b]], (label, b)
        assert np.all(k[b, d["rows"][b, :m]] > 0) and np.all(d["rows"][b, m:] == -1), (label, b)
        assert abs(d["family_share"][b].sum() - 1.0) <= 1e-12 and np.all(d["family_share"][b, nf:] == 0), (label, b)
        for q in range(1, int(d["n_found"][b]) + 1):
            med, lab = d["medoid"][b, q - 1, :q], d["label"][b, q - 1, :m]
            assert abs(d["share"][b, q - 1].sum() - 1.0) <= 1e-12 and np.all(lab >= 0) and np.all(lab < q), (label, b, q)
            to = D[med][:, :m]                                                 # the medoids' rows
            assert np.array_equal(d["nearest"][b, q - 1, :m], to.min(axis=0)) and np.array_equal(d["nearest"][b, q - 1, :m], to[lab, np.arange(m)]), (label, b, q)
        assert np.all(d["family_label"][b, :m] >= 0) and np.all(d["family_label"][b, m:] == -1), (label, b)
        share = d["family_chain_share"][b]                                     # [Q, C]
        used = np.unique(d["chain_of"][b, :m])
        assert share.shape[1] == C and np.allclose(share[:, used].sum(axis=0), 1.0, rtol=0, atol=1e-12), (label, b)
        assert np.isnan(share[:, np.setdiff1d(np.arange(C), used)]).all(), (label, b)
    assert some, label


def test_families_of_real_chains_and_of_replicates():
    from geobipy_amd import replicates
    B, nk, thin = 16, 32, 2
    _, _, dc = _chains(B, 17, exact=True, hitmap=True, ensemble=dict(n_keep=nk, thin=thin))
    dc.run(60, accumulate=False)
    dc.run(nk * thin)
    z1 = float(dc.n_depth_bins * dc.depth_bin_width)
    ens = ensembles.from_chains(dc)
    d = _numpy(families.families(ens, z1, keep_distance=True))
    assert d["distance"].shape == (B, nk, nk) and np.all(d["n_used"] == nk)
    _consistent(d, ens, 1, "real chains")
    want = families.distance_reference(ens.k[3].cpu().numpy(), ens.edges[3].cpu().numpy(), ens.sigma[3].cpu().numpy(), d["rows"][3], 0.0, z1, dtype=np.longdouble)
    assert np.allclose(d["distance"][3], want.astype(np.float64), rtol=1e-12, atol=1e-13)
    lg = _numpy(families.families(ens, z1, z0=1.0, measure="log", max_models=10, keep_distance=True))      # thinned: stride 4, 8 models
    assert np.all(lg["n_used"] == 8) and np.array_equal(lg["rows"][0], np.arange(0, nk, 4))
    _consistent(lg, ens, 1, "real chains, log measure")
    none = _numpy(families.families(ens._replace(k=ens.k[:0], edges=ens.edges[:0], sigma=ens.sigma[:0]), z1, keep_distance=True))      # an empty block
    assert none["distance"].shape == (0, 1, 1) and none["n_families"].shape == (0,) and none["family_edges"].shape == (0, 4, ens.edges.shape[2])
    pooled = ensembles.from_chains(replicates.Pooled(dc, 2))
    p = _numpy(families.families(pooled, z1, chains=2, keep_distance=True))
    assert p["distance"].shape == (B // 2, 2 * nk, 2 * nk) and p["family_chain_share"].shape == (B // 2, 4, 2)
    assert np.array_equal(p["chain_of"][0], np.repeat([0, 1], nk))
    _consistent(p, pooled, 2, "replicates")


def test_families_of_time_domain_chains():
    from geobipy_amd.tdem import TdemDeviceChains
    from test_tdem_sampler import OFFSET, _survey
    s, h, data, scale, opts, groups = _survey(4, seed=3)
    dc = TdemDeviceChains(s, h, data, OFFSET, seed=77, hitmap=True, ensemble=dict(n_keep=32, thin=4), **opts)
    dc.run(100, accumulate=False)
    dc.run(120)
    ens = ensembles.from_chains(dc)
    d = _numpy(families.families(ens, float(dc.n_depth_bins * dc.depth_bin_width), keep_distance=True))
    assert np.all(d["n_used"] == 30)
    _consistent(d, ens, 1, "time domain")


def test_survey_and_command_lines_carry_the_families(tmp_path):
    from geobipy_amd import survey
    from geobipy_amd.__main__ import main
    options = os.path.join(GOLDEN, "resolve_options_small")
    timings = {}
    res = survey.infer(options, exact_jacobian=True, ensemble=16, ensemble_families=dict(max_families=3), timings=timings)
    off = survey.infer(options, exact_jacobian=True, ensemble=16)
    S, K = res["status"].size, res["ensemble_edges"].shape[2]
    new = ("ensemble_families_n", "ensemble_family_share", "ensemble_family_silhouette", "ensemble_family_k", "ensemble_family_edges",
           "ensemble_family_sigma", "ensemble_central_k", "ensemble_central_edges", "ensemble_central_sigma", "ensemble_central_mean_distance")
    assert set(res) - set(off) == set(new) and set(off) - set(res) == set() and "ensemble" in timings
    for n in off:
        assert np.array_equal(np.asarray(res[n]), np.asarray(off[n]), equal_nan=True), n       # keyword off: the arrays of before
    assert res["ensemble_families_n"].shape == (S,) and res["ensemble_families_n"].dtype == np.int32 and res["ensemble_central_k"].dtype == np.int32
    assert res["ensemble_family_share"].shape == res["ensemble_family_silhouette"].shape == res["ensemble_family_k"].shape == (S, 3)
    assert res["ensemble_family_edges"].shape == res["ensemble_family_sigma"].shape == (S, 3, K)
    assert res["ensemble_central_edges"].shape == res["ensemble_central_sigma"].shape == (S, K) and res["ensemble_central_mean_distance"].shape == (S,)
    usable = (res["ensemble_k"] > 0).sum(axis=1) >= 8
    assert usable.any() and np.all(res["ensemble_families_n"][usable] >= 1) and np.all(res["ensemble_families_n"][~usable] == 0)
    assert np.all(res["ensemble_central_k"][usable] >= 1) and np.all(res["ensemble_central_mean_distance"][usable] >= 0)
    for s in np.nonzero(usable)[0][:3]:                                          # the central model is one of the kept models
        kc = res["ensemble_central_k"][s]
        hit = [t for t in range(res["ensemble_k"].shape[1]) if res["ensemble_k"][s, t] == kc
               and np.array_equal(res["ensemble_edges"][s, t], res["ensemble_central_edges"][s])
               and np.array_equal(res["ensemble_sigma"][s, t], res["ensemble_central_sigma"][s], equal_nan=True)]
        assert hit, s
        assert abs(res["ensemble_family_share"][s].sum() - 1.0) <= 1e-12
    # the survey's command line, with replicates
    out = tmp_path / "cli"
    out.mkdir()
    assert main([options, str(out), "--exact-jacobian", "--no-containers", "--ensemble", "16", "--ensemble-families", "2", "--replicates", "2"]) == 0
    ln = np.unique(res["line"])[0]
    line = np.load(str(out / "{}.npz".format(ln)))
    n_line = int((res["line"] == ln).sum())
    assert all(n in line.files for n in new) and line["ensemble_family_share"].shape == (n_line, 2) and line["ensemble_families_n"].shape == (n_line,)
    # the module's command line on a saved ensemble
    _, _, dc = _chains(6, 5, exact=True, hitmap=True, ensemble=dict(n_keep=24, thin=2))
    dc.run(30, accumulate=False)
    dc.run(48)
    ens = ensembles.from_chains(dc)
    path = ensembles.save(ens, str(tmp_path / "run.npz"))
    written = families.main([path, "--depth", "120", "--from", "2", "--measure", "log", "--max-families", "3"])
    assert written == str(tmp_path / "run.families.npz")
    f = np.load(written)
    want = _numpy(families.families(ens, 120.0, z0=2.0, measure="log", max_families=3))
    assert all(np.array_equal(f[n], want[n], equal_nan=True) for n in want) and int(f["thin"]) == 2 and str(f["measure"]) == "log" and float(f["z0"]) == 2.0


def test_the_c_entries_refuse_bad_arguments_by_name():
    from geobipy_amd import _lib
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    B, ns, K, n, Q = 2, 6, 4, 5, 3
    k = torch.ones((B, ns), dtype=torch.int32, device=dev)
    e = torch.full((B, ns, K), float("inf"), dtype=torch.float64, device=dev)
    s = torch.ones((B, ns, K), dtype=torch.float64, device=dev)
    rows = torch.zeros((B, n), dtype=torch.int32, device=dev)
    dist = torch.full((B, n, n), 7.0, dtype=torch.float64, device=dev)
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    distance = lambda B_=B, ns_=ns, K_=K, k_=k, e_=e, s_=s, n_=n, rows_=rows, z0=0.0, z1=10.0, measure=0, dist_=dist: lib.gbp_ensemble_distance(      # noqa: E731
        B_, ns_, K_, p(k_), p(e_), p(s_), n_, p(rows_), z0, z1, measure, 1, 0, p(dist_), st)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(B_=-1), dict(ns_=0), dict(K_=0), dict(K_=65), dict(n_=0), dict(n_=4097), dict(z0=-1.0), dict(z1=0.0), dict(z0=10.0), dict(z1=inf),
               dict(z0=nan), dict(z1=nan), dict(measure=2), dict(measure=-1), dict(measure=1), dict(k_=None), dict(e_=None), dict(s_=None),
               dict(rows_=None), dict(dist_=None), dict(B_=2 ** 16, n_=4096), dict(B_=2 ** 24), dict(B_=2 ** 9, n_=4096)):
        assert distance(**kw) != 0 and b"gbp_ensemble_distance" in lib.gbp_last_error(), kw
    assert distance(B_=0, k_=None) == 0                                  # an empty block: OK without a launch
    n_used = torch.full((B,), n, dtype=torch.int32, device=dev)
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=dev)      # noqa: E731
    medoid, label, iterations, n_found = i32(B, Q, Q), i32(B, Q, n), i32(B, Q), i32(B)
    nearest, second = torch.full((B, Q, n), 7.0, dtype=torch.float64, device=dev), torch.full((B, Q, n), 7.0, dtype=torch.float64, device=dev)
    conv = torch.full((B, Q), 7, dtype=torch.uint8, device=dev)
    fam = lambda B_=B, n_=n, dist_=dist, nu=n_used, Q_=Q, it=5, med=medoid, lab=label, near=nearest, sec=second, its=iterations, cv=conv, nf=n_found: \
        lib.gbp_distance_families(B_, n_, p(dist_), p(nu), Q_, it, p(med), p(lab), p(near), p(sec), p(its), p(cv), p(nf), st)      # noqa: E731
    for kw in (dict(B_=-1), dict(n_=0), dict(n_=4097), dict(Q_=0), dict(Q_=9), dict(it=-1), dict(dist_=None), dict(nu=None), dict(med=None),
               dict(lab=None), dict(near=None), dict(sec=None), dict(its=None), dict(cv=None), dict(nf=None), dict(B_=2 ** 24)):
        assert fam(**kw) != 0 and b"gbp_distance_families" in lib.gbp_last_error(), kw
    assert fam(B_=0, dist_=None) == 0
    torch.cuda.synchronize()
    assert torch.all(dist == 7.0) and torch.all(medoid == 7) and torch.all(label == 7) and torch.all(nearest == 7.0) and torch.all(second == 7.0)
    assert torch.all(iterations == 7) and torch.all(conv == 7) and torch.all(n_found == 7)       # nothing was written
