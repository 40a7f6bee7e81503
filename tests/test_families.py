"""The host side of the model families (geobipy_amd/families.py): the two rules ``distance_reference`` and
``families_reference`` against closed forms, a brute-force raster and hand matrices; ``select`` on planted families; ``used_rows``
against ``ensembles.segments``; every refusal that comes before the library loads; the argument checks of the survey driver."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, ensembles, families

U = 2.0 ** -52


def _ensemble(models, K):
    """k, edges, sigma of hand-made models [(interfaces, log10 values)]; None: an empty slot."""
    n = len(models)
    k, edges, sigma = np.zeros(n, dtype=np.int32), np.full((n, K), np.inf), np.full((n, K), np.nan)
    for i, m in enumerate(models):
        if m is None:
            continue
        e, a = m
        k[i] = len(a)
        edges[i, :len(e)] = e
        sigma[i, :len(a)] = 10.0 ** np.asarray(a, dtype=np.float64)
    return k, edges, sigma


def _stored(models, K):
    """The same with the values stored as they are (``stored=True``)."""
    k, edges, sigma = _ensemble(models, K)
    for i, m in enumerate(models):
        if m is not None:
            sigma[i, :len(m[1])] = m[1]
    return k, edges, sigma


def planted(tops, seed, n=96, K=4):
    """``n`` two-layer models, model i with its interface at tops[i mod len(tops)] +- 1 m and the values -2.0 / -0.5 +- 0.05 decades:
    (k, edges, sigma, the planted family of every model)."""
    rng = np.random.default_rng(seed)
    which = np.arange(n) % len(tops)
    k = np.full(n, 2, dtype=np.int32)
    edges, sigma = np.full((n, K), np.inf), np.full((n, K), np.nan)
    edges[:, 0] = np.asarray(tops, dtype=np.float64)[which] + rng.uniform(-1.0, 1.0, n)
    sigma[:, 0] = 10.0 ** (-2.0 + rng.uniform(-0.05, 0.05, n))
    sigma[:, 1] = 10.0 ** (-0.5 + rng.uniform(-0.05, 0.05, n))
    return k, edges, sigma, which


PLANTED = ([40.0], [30.0, 60.0], [20.0, 50.0, 90.0])


def same_partition(label, which):
    """The labels reproduce the planted partition exactly."""
    pairs = set(zip(label.tolist(), which.tolist()))
    return len(pairs) == len(set(which.tolist())) == len(set(label.tolist()))


def stages_of(results):
    """The dict ``summaries`` and ``select`` take, from a list of ``families_reference`` results (one per sounding), with the summaries."""
    st = {n: torch.as_tensor(np.stack([np.asarray(r[n]) for r in results])) for n in ("medoid", "label", "nearest", "second", "iterations", "converged")}
    st["n_found"] = torch.tensor([r["n_found"] for r in results], dtype=torch.int32)
    st["cost"], st["silhouette"], st["share"] = families.summaries(st)
    return st


# ---- the distance --------------------------------------------------------------------------------------------------------------------

def test_two_layer_pair_in_closed_form():
    t1, t2, a, b, z0, z1 = 31.0, 47.5, -2.25, -0.5, 3.0, 120.0
    # above t1 and below t2 the two models agree; between them they differ by (a - b)
    k, e, s = _stored([([t1], [a, b]), ([t2], [a, b])], 3)
    for dtype in (np.float64, np.longdouble):
        D2 = families.distance_reference(k, e, s, [0, 1], z0, z1, stored=True, squared=True, dtype=dtype)
        want = (t2 - t1) * (a - b) ** 2 / (z1 - z0)
        assert abs(float(D2[0, 1]) - want) <= 8 * U * want and D2[0, 1] == D2[1, 0] and D2[0, 0] == 0 and D2[1, 1] == 0
        D = families.distance_reference(k, e, s, [0, 1], z0, z1, stored=True, dtype=dtype)
        assert abs(float(D[0, 1]) - np.sqrt(want)) <= 8 * U * np.sqrt(want)
        L2 = families.distance_reference(k, e, s, [0, 1], z0, z1, measure="log", stored=True, squared=True, dtype=dtype)
        want = np.log(t2 / t1) * (a - b) ** 2 / np.log(z1 / z0)
        assert abs(float(L2[0, 1]) - want) <= 16 * U * want
    # log10 of the stored conductivities is what the default compares
    k, e, s = _ensemble([([t1], [a, b]), ([t2], [a, b])], 3)
    D2 = families.distance_reference(k, e, s, [0, 1], z0, z1, squared=True)
    assert abs(D2[0, 1] - (t2 - t1) * (a - b) ** 2 / (z1 - z0)) <= 64 * U * D2[0, 1]


def test_distance_against_a_brute_force_raster():
    rng = np.random.default_rng(5)
    K, n, z0, z1, cells = 7, 6, 2.0, 90.0, 20000
    models = [(np.sort(rng.uniform(0.0, 100.0, kk - 1)), rng.uniform(-3.0, 0.0, kk)) for kk in rng.integers(1, K + 1, n)]
    k, e, s = _stored(models, K)
    width = (z1 - z0) / cells
    z = z0 + (np.arange(cells) + 0.5) * width
    x = np.stack([np.asarray(a)[np.searchsorted(ed, z, side="right")] for ed, a in models])
    jump = max(float(np.ptp(np.concatenate([a for _, a in models]))), 1.0) ** 2
    for measure, w in (("linear", np.full(cells, 1.0 / cells)), ("log", np.log((z + 0.5 * width) / (z - 0.5 * width)) / np.log(z1 / z0))):
        D2 = families.distance_reference(k, e, s, np.arange(n), z0, z1, measure=measure, stored=True, squared=True)
        raster = ((x[:, None, :] - x[None, :, :]) ** 2 * w).sum(axis=2)
        # a cell that holds an interface is wrong by at most its weight times the largest squared jump; at most 2 (K - 1) such cells
        assert np.all(np.abs(D2 - raster) <= 2 * (K - 1) * w.max() * jump + 1e-12)
        assert np.abs(D2 - raster).max() > 0


def test_identical_models_edge_cases_and_absent_rows():
    z0, z1 = 10.0, 50.0
    models = [([20.0, 30.0], [-1.0, -2.0, -3.0]),
              ([20.0, 30.0], [-1.0, -2.0, -3.0]),                      # another slot that holds the same model
              ([10.0, 50.0], [-7.0, -2.0, 4.0]),                       # interfaces exactly at z0 and z1: only the middle layer counts
              ([20.0, 35.0], [-1.0, -2.5, -3.0]),                      # shares the interface at 20 with model 0
              ([1.0, 9.999], [5.0, 6.0, -2.0]),                        # every interface above z0: the last layer
              ([50.001, 70.0], [-2.0, 5.0, 6.0]),                      # every interface below z1: the first layer
              ([], [-2.0]),                                            # k = 1
              None]                                                    # an empty slot
    k, e, s = _stored(models, 4)
    rows = [0, 1, 2, 3, 4, 5, 6, 7, -1, 8, 0]
    for measure in ("linear", "log"):
        D2 = families.distance_reference(k, e, s, rows, z0, z1, measure=measure, stored=True, squared=True)
        assert D2[0, 1] == 0.0 and D2[0, 10] == 0.0 and D2[1, 10] == 0.0          # identical models, one slot listed twice
        assert np.all(D2[[2, 4, 5, 6]][:, [2, 4, 5, 6]] == 0.0)                   # four ways to be -2 on the whole window
        absent = np.array([7, 8, 9])
        assert np.isnan(D2[absent]).all() and np.isnan(D2[:, absent]).all()
        present = np.setdiff1d(np.arange(len(rows)), absent)
        assert np.isfinite(D2[np.ix_(present, present)]).all() and np.all(np.diag(D2)[present] == 0.0)
        assert np.array_equal(D2, D2.T, equal_nan=True)
        mu = (lambda p, q: np.log(q / p)) if measure == "log" else (lambda p, q: q - p)
        want = (mu(10.0, 20.0) * 1.0 + mu(30.0, 50.0) * 1.0) / mu(z0, z1)          # model 0 against -2: (-1 + 2)^2 and (-3 + 2)^2
        assert abs(D2[0, 6] - want) <= 16 * U * want
        want = (mu(20.0, 30.0) * 0.25 + mu(30.0, 35.0) * 0.25) / mu(z0, z1)        # model 0 against model 3: 0.5 apart on [20, 35)
        assert abs(D2[0, 3] - want) <= 16 * U * want
    # an interface exactly at z0 gives the layer below: model (z0,) differs from its upper value on the whole window
    k, e, s = _stored([([z0], [1.0, 2.0]), ([], [2.0]), ([], [1.0])], 2)
    D = families.distance_reference(k, e, s, [0, 1, 2], z0, z1, stored=True)
    assert D[0, 1] == 0.0 and D[0, 2] == 1.0


def test_float64_evaluation_against_long_double():
    rng = np.random.default_rng(11)
    K, n = 64, 9
    models = [(np.sort(rng.uniform(0.0, 300.0, kk - 1)), rng.uniform(-4.0, 1.0, kk)) for kk in [64, 64, 1, 2, 33, 64, 17, 5, 64]]
    k, e, s = _ensemble(models, K)
    for measure, z0 in (("linear", 0.0), ("log", 1.5)):
        lo = families.distance_reference(k, e, s, np.arange(n), z0, 250.0, measure=measure, squared=True)
        hi = families.distance_reference(k, e, s, np.arange(n), z0, 250.0, measure=measure, squared=True, dtype=np.longdouble)
        amax = 4.0
        bound = (2 * K + 24) * U * hi + 16 * U * amax * np.sqrt(hi) + (8 * U * amax) ** 2
        assert lo.dtype == np.float64 and hi.dtype == np.longdouble and np.all(np.abs(lo - hi) <= bound)


def test_distance_reference_refuses():
    k, e, s = _ensemble([([5.0], [0.0, 1.0])], 2)
    for kw in (dict(z0=-1.0), dict(z1=0.0), dict(z1=float("inf")), dict(z0=float("nan")), dict(measure="sqrt"), dict(measure="log")):
        with pytest.raises(ValueError):
            families.distance_reference(k, e, s, [0], **dict(dict(z0=0.0, z1=10.0), **kw))


# ---- the clustering ------------------------------------------------------------------------------------------------------------------

def _line(points):
    p = np.asarray(points, dtype=np.float64)
    return np.abs(p[:, None] - p[None, :])


def test_stage_one_and_its_tie():
    r = families.families_reference(_line([0.0, 1.0, 2.0, 3.0]), 4, 1, 10)       # column sums 6 4 4 6: the lower of the two
    assert r["n_found"] == 1 and r["medoid"].tolist() == [[1]] and r["label"].tolist() == [[0, 0, 0, 0]]
    assert r["nearest"].tolist() == [[1.0, 0.0, 1.0, 2.0]] and np.isnan(r["second"]).all()
    assert r["iterations"].tolist() == [1] and r["converged"].tolist() == [1]


def test_hand_matrices_with_ties():
    D = _line([0.0, 1.0, 5.0, 6.0])                                              # column sums 12 10 10 12: medoid 1 (lowest of equals)
    r = families.families_reference(D, 4, 3, 10)
    assert r["medoid"][0].tolist() == [1, -1, -1]
    # stage 2: nearest = 1 0 4 5; gains: c=0: 1; c=1: 0; c=2: 4 + 4 = 8; c=3: 3 + 5 = 8 -> 2, the lower of two equals
    # assignment: 0, 1 -> family 0, 2, 3 -> family 1; update: family 0 sums 1 1 -> 0 (lowest), family 1 sums 1 1 -> 2; the medoids
    # changed (1 -> 0), a second update confirms them
    assert r["medoid"][1].tolist() == [0, 2, -1] and r["label"][1].tolist() == [0, 0, 1, 1]
    assert r["iterations"][1] == 2 and r["converged"][1] == 1
    assert r["nearest"][1].tolist() == [0.0, 1.0, 0.0, 1.0] and r["second"][1].tolist() == [5.0, 4.0, 5.0, 6.0]
    # stage 3: nearest = 0 1 0 1; gains 0 1 0 1 -> 1, the lower of two equals
    assert r["n_found"] == 3 and r["medoid"][2].tolist() == [0, 2, 1] and r["label"][2].tolist() == [0, 2, 1, 1]
    # max_iter = 0 and 1 on three points: the gains of stage 2 are 2 0 2 -> candidate 0, the lower of two equals (no model is tied here)
    D = _line([0.0, 2.0, 4.0])
    r = families.families_reference(D, 3, 2, 0)                                  # max_iter = 0: the new medoid and one assignment
    assert r["medoid"][0].tolist() == [1, -1] and r["medoid"][1].tolist() == [1, 0]       # gains 2 0 2 -> 0
    assert r["label"][1].tolist() == [1, 0, 0] and r["iterations"].tolist() == [0, 0] and r["converged"].tolist() == [0, 0]
    r = families.families_reference(D, 3, 2, 1)                                  # one update: family 0 = {1, 2} keeps 1, family 1 = {0} keeps 0
    assert r["medoid"][1].tolist() == [1, 0] and r["iterations"].tolist() == [1, 1] and r["converged"].tolist() == [1, 1]


def test_a_model_between_two_medoids_goes_to_the_one_that_joined_first():
    """Points 0, 2, 4, 1 on a line.  Column sums 7 5 9 5: medoid 1 (x = 2), the lower of two equals.  Stage 2: nearest = 2 0 2 1, gains
    c=0: 2 + 0 = 2, c=1: 0, c=2: 2, c=3: 1 + 1 = 2 -> candidate 0 (x = 0), the lowest of three equals: the medoids are [1, 0], so the one
    that joined first has the HIGHER model index.  Model 3 (x = 1) is 1 away from both: it goes to position 0 (model 1, joined first),
    and its second-nearest distance equals its nearest."""
    D = _line([0.0, 2.0, 4.0, 1.0])
    for max_iter, iterations, converged in ((0, [0, 0], [0, 0]), (10, [1, 1], [1, 1])):
        r = families.families_reference(D, 4, 2, max_iter)
        assert r["n_found"] == 2 and r["medoid"][0].tolist() == [1, -1] and r["medoid"][1].tolist() == [1, 0]
        assert D[1, 3] == D[0, 3] == 1.0                                         # the tie: model 3 against the two medoids
        assert r["label"][1].tolist() == [1, 0, 0, 0]                            # model 3 -> position 0, not position 1
        assert r["nearest"][1].tolist() == [0.0, 0.0, 2.0, 1.0] and r["second"][1].tolist() == [2.0, 2.0, 4.0, 1.0]
        assert r["second"][1, 3] == r["nearest"][1, 3]
        # the update: family 0 = {1, 2, 3} has the sums 3 5 4 -> model 1 stays, family 1 = {0} keeps model 0: one update confirms them
        assert r["iterations"].tolist() == iterations and r["converged"].tolist() == converged
    # the same points listed so that the medoid that joined first has the lower index as well: the label is again position 0
    r = families.families_reference(_line([2.0, 0.0, 4.0, 1.0]), 4, 2, 10)       # sums 5 7 9 5 -> 0; gains 0 2 2 2 -> 1
    assert r["medoid"][1].tolist() == [0, 1] and r["label"][1].tolist() == [0, 1, 0, 0] and r["second"][1, 3] == r["nearest"][1, 3] == 1.0


def test_two_distinct_models_twice_give_two_families():
    D = np.array([[0.0, 3.0, 0.0, 3.0], [3.0, 0.0, 3.0, 0.0], [0.0, 3.0, 0.0, 3.0], [3.0, 0.0, 3.0, 0.0]])
    r = families.families_reference(D, 4, 4, 100)
    assert r["n_found"] == 2 and r["medoid"][1].tolist() == [0, 1, -1, -1] and r["label"][1].tolist() == [0, 1, 0, 1]
    assert r["nearest"][1].tolist() == [0.0] * 4 and r["second"][1].tolist() == [3.0] * 4
    assert np.all(r["medoid"][2:] == -1) and np.all(r["label"][2:] == -1) and np.isnan(r["nearest"][2:]).all()
    assert r["iterations"][2:].tolist() == [0, 0] and r["converged"][2:].tolist() == [0, 0]
    st = stages_of([r])
    assert st["silhouette"][0, 1] == 1.0 and st["share"][0, 1].tolist() == [0.5, 0.5, 0.0, 0.0] and torch.isnan(st["share"][0, 2]).all()
    assert families.select(st).tolist() == [2]


def test_one_model_a_prefix_a_nan_and_no_iterations():
    r = families.families_reference(np.zeros((1, 1)), 1, 3, 5)
    assert r["n_found"] == 1 and r["medoid"][0].tolist() == [0, -1, -1] and r["label"][:, 0].tolist() == [0, -1, -1] and r["nearest"][0, 0] == 0.0
    D = _line([0.0, 1.0, 10.0, 11.0, 50.0])
    part = families.families_reference(D, 4, 2, 10)                              # n_used < n: model 4 does not count
    whole = families.families_reference(D[:4, :4], 4, 2, 10)
    assert part["label"][:, 4].tolist() == [-1, -1] and np.isnan(part["nearest"][:, 4]).all()
    for name in ("label", "nearest", "second"):
        assert np.array_equal(part[name][:, :4], whole[name], equal_nan=True)
    assert np.array_equal(part["medoid"], whole["medoid"]) and part["n_found"] == whole["n_found"] == 2
    assert families.families_reference(D, 99, 1, 1)["n_found"] == 1 and families.families_reference(D, -3, 1, 1)["n_found"] == 0
    for bad in (np.nan, np.inf, -1.0):
        B = D.copy()
        B[1, 2] = bad
        r = families.families_reference(B, 4, 2, 10)
        assert r["n_found"] == 0 and np.all(r["medoid"] == -1) and np.all(r["label"] == -1) and np.isnan(r["nearest"]).all()
        B = D.copy()
        B[1, 4] = bad                                                            # outside the prefix: not looked at
        assert families.families_reference(B, 4, 2, 10)["n_found"] == 2
    for kw in (dict(q_max=0), dict(q_max=9), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            families.families_reference(D, 4, **dict(dict(q_max=2, max_iter=3), **kw))
    with pytest.raises(ValueError):
        families.families_reference(np.zeros((2, 3)), 2, 1, 1)


def test_the_sums_keep_the_order_of_the_rule():
    """numpy's cumsum is the loop ``for j in range(n): s += D[j, i]``: the bits the device is held to."""
    rng = np.random.default_rng(3)
    D = rng.uniform(0.0, 1.0, (40, 40))
    D = D + D.T
    np.fill_diagonal(D, 0.0)
    s = np.zeros(40)
    for j in range(40):
        s = s + D[j]
    assert np.array_equal(np.cumsum(D, axis=0)[-1], s)
    r = families.families_reference(D, 40, 1, 1)
    assert r["medoid"][0, 0] == int(np.argmin(s))


@pytest.mark.parametrize("seed", [1, 2])
def test_planted_families_are_recovered_and_selected(seed):
    results = []
    for tops in PLANTED:
        k, e, s, which = planted(tops, seed)
        D = families.distance_reference(k, e, s, np.arange(k.size), 0.0, 150.0)
        r = families.families_reference(D, k.size, 4, 100)
        assert r["n_found"] == 4 and r["converged"].all()
        assert same_partition(r["label"][len(tops) - 1], which), tops
        results.append(r)
    st = stages_of(results)
    sil = st["silhouette"].numpy()
    print("silhouettes", np.round(sil, 3).tolist())
    assert np.isnan(sil[:, 0]).all() and np.all(sil[0, 1:] < 0.6) and sil[1, 1] > 0.8 and sil[2, 2] > 0.8
    assert families.select(st).tolist() == [1, 2, 3]
    assert families.select({n: v.numpy() for n, v in st.items()}).tolist() == [1, 2, 3]        # numpy in, numpy out
    assert families.select(st, min_silhouette=0.3).tolist() == [2, 2, 3] and families.select(st, min_share=0.6).tolist() == [1, 1, 1]
    assert np.allclose(st["share"][2, 2, :3].numpy(), 1.0 / 3.0) and np.allclose(st["cost"][:, 0].numpy(), [r["nearest"][0].sum() for r in results])
    for kw in (dict(min_silhouette=1.5), dict(min_share=-0.1), dict(min_share=True)):
        with pytest.raises(ValueError):
            families.select(st, **kw)


# ---- which models --------------------------------------------------------------------------------------------------------------------

def test_used_rows_against_segments():
    Ens = ensembles.Ensemble
    per, C = 20, 3
    count = np.array([[20, 20, 20], [20, 7, 13], [3, 0, 7], [9, 20, 8]])         # chains with fewer than 8 filled slots are left out
    k = np.zeros((4, C * per), dtype=np.int32)
    for b in range(4):
        for c in range(C):
            k[b, c * per:c * per + count[b, c]] = 2
    ens = Ens(k, None, None, None, None, 1, None)
    start, seg_m, seg_n, used = ensembles.segments(count, per)
    rows, n_used, chain_of = families.used_rows(ens, chains=C, max_models=4096)
    assert rows.dtype == n_used.dtype == chain_of.dtype == np.int32 and rows.shape == chain_of.shape == (4, 60)
    for b in range(4):
        want = np.concatenate([np.arange(start[b, m], start[b, m] + seg_n[b]) for m in range(seg_m[b])] + [np.zeros(0, dtype=np.int64)])
        assert n_used[b] == want.size == used[b] * 2 * seg_n[b]
        assert np.array_equal(rows[b, :n_used[b]], want) and np.all(rows[b, n_used[b]:] == -1)
        assert np.array_equal(chain_of[b, :n_used[b]], want // per) and np.all(chain_of[b, n_used[b]:] == -1)
    assert n_used.tolist() == [60, 24, 0, 24]
    rows, n_used, chain_of = families.used_rows(ens, chains=C, max_models=25)    # strides 3, 1, -, 1
    assert n_used.tolist() == [20, 24, 0, 24] and rows.shape == (4, 24) and np.array_equal(rows[0, :20], np.arange(0, 60, 3))
    t = families.used_rows(Ens(torch.as_tensor(k), None, None, None, None, 1, None), chains=C, max_models=25)
    assert all(torch.is_tensor(a) and a.dtype == torch.int32 for a in t) and np.array_equal(t[0].numpy(), rows)
    empty = families.used_rows(Ens(np.zeros((2, 6), dtype=np.int32), None, None, None, None, 1, None))
    assert empty[0].shape == (2, 1) and empty[1].tolist() == [0, 0]
    for kw in (dict(chains=0), dict(chains=7), dict(max_models=0), dict(max_models=4097), dict(max_models=2.5)):
        with pytest.raises(ValueError):
            families.used_rows(ens, **dict(dict(chains=C, max_models=10), **kw))


# ---- refusals before the library loads -----------------------------------------------------------------------------------------------

def _host_ensemble(B=2, ns=16, K=3):
    k = torch.full((B, ns), 2, dtype=torch.int32)
    edges = torch.full((B, ns, K), float("inf"), dtype=torch.float64)
    edges[:, :, 0] = 5.0
    sigma = torch.full((B, ns, K), 0.1, dtype=torch.float64)
    return ensembles.Ensemble(k, edges, sigma, torch.ones((B, ns), dtype=torch.float64), (k > 0).sum(dim=1), 1, torch.zeros(B, dtype=torch.float64))


def test_the_entries_refuse_in_order_and_never_fall_back(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    ens = _host_ensemble()
    rows = torch.zeros((2, 4), dtype=torch.int32)
    # tensors first
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        families.distance(ens._replace(k=ens.k.numpy()), rows, 0.0, 10.0)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        families.distance(ens, rows.numpy(), 0.0, 10.0)
    # then shapes, dtypes, values -- on host tensors, so before the device check
    for bad in (dict(k=ens.k[:, :3]), dict(edges=ens.edges[:, :, :2]), dict(sigma=ens.sigma[0])):
        with pytest.raises(ValueError, match="ensemble"):
            families.distance(ens._replace(**bad), rows, 0.0, 10.0)
    for bad_rows in (rows[0], rows[:1], torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 4097), dtype=torch.int32)):
        with pytest.raises(ValueError, match="rows"):
            families.distance(ens, bad_rows, 0.0, 10.0)
    with pytest.raises(TypeError):
        families.distance(ens, rows.long(), 0.0, 10.0)
    with pytest.raises(TypeError):
        families.distance(ens._replace(sigma=ens.sigma.float()), rows, 0.0, 10.0)
    big = torch.zeros((1, 2, 65), dtype=torch.float64)
    with pytest.raises(ValueError, match="K in"):
        families.distance(ens._replace(k=torch.zeros((1, 2), dtype=torch.int32), edges=big, sigma=big), rows[:1], 0.0, 10.0)
    for kw in (dict(z0=-1.0), dict(z1=0.0), dict(z1=float("nan")), dict(measure="cubic"), dict(measure="log"), dict(block=0), dict(block=1.5)):
        with pytest.raises(ValueError):
            families.distance(ens, rows, **dict(dict(z0=0.0, z1=10.0), **kw))
    # the device last
    with pytest.raises(_lib.NativeLibraryError, match="gbp_ensemble_distance"):
        families.distance(ens, rows, 0.0, 10.0)

    D, n_used = torch.zeros((2, 4, 4), dtype=torch.float64), torch.full((2,), 4, dtype=torch.int32)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        families.cluster(D.numpy(), n_used)
    for bad in ((D[0], n_used), (D[:, :3], n_used), (D, n_used[:1]), (torch.zeros((2, 4097, 4097), dtype=torch.float64)[:0], n_used)):
        with pytest.raises(ValueError, match="dist"):
            families.cluster(*bad)
    with pytest.raises(TypeError):
        families.cluster(D.float(), n_used)
    with pytest.raises(TypeError):
        families.cluster(D, n_used.long())
    for kw in (dict(max_families=0), dict(max_families=9), dict(max_families=2.0), dict(max_iter=-1), dict(max_iter=True)):
        with pytest.raises(ValueError):
            families.cluster(D, n_used, **kw)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_distance_families"):
        families.cluster(D, n_used)

    for kw in (dict(z1=0.0), dict(z0=3.0, z1=2.0), dict(measure="log"), dict(max_families=9), dict(chains=3), dict(max_models=0), dict(block=-1)):
        with pytest.raises(ValueError):
            families.families(ens, **dict(dict(z1=10.0), **kw))
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        families.families(ens._replace(k=ens.k.numpy()), 10.0)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        families.families(ens, 10.0)


def test_the_command_line_refuses_before_any_device_work(capsys):
    path, kw, device = families.parse_args(["run.npz", "--depth", "150", "--from", "2", "--measure", "log", "--chains", "2", "--max-families", "3"])
    assert path == "run.npz" and kw == dict(z1=150.0, z0=2.0, measure="log", chains=2, max_families=3, max_models=1024) and device == "cuda:0"
    assert families.families_path("a/run.npz") == "a/run.families.npz" and families.families_path("run") == "run.families.npz"
    for argv in (["run.npz"], ["run.npz", "--depth", "0"], ["run.npz", "--depth", "10", "--measure", "log"], ["run.npz", "--depth", "10", "--from", "10"],
                 ["run.npz", "--depth", "10", "--max-families", "9"], ["run.npz", "--depth", "10", "--chains", "0"],
                 ["run.npz", "--depth", "10", "--max-models", "5000"]):
        with pytest.raises(SystemExit):
            families.parse_args(argv)
    capsys.readouterr()


def test_the_survey_driver_checks_the_keyword():
    from geobipy_amd import survey_run
    from geobipy_amd.__main__ import parse
    check = survey_run.ensemble_families_argument
    assert check(False, None) is None and check(None, 16) is None
    assert check(True, 16) == dict(max_families=4, max_models=1024, measure="linear", min_silhouette=0.7)
    assert check(dict(max_families=2, min_silhouette=0.5), 16) == dict(max_families=2, max_models=1024, measure="linear", min_silhouette=0.5)
    for no_ensemble in (None, False):
        with pytest.raises(ValueError, match="needs ensemble"):
            check(True, no_ensemble)
    for bad in (3, "yes", dict(families=2), dict(max_families=0), dict(max_families=9), dict(max_families=2.0), dict(max_models=0),
                dict(max_models=4097), dict(measure="cubic"), dict(measure="log"), dict(min_silhouette=1.5), dict(min_silhouette="high")):
        with pytest.raises(ValueError, match="ensemble_families"):
            check(bad, 16)
    a = parse(["options", "out", "--ensemble", "16", "--ensemble-families"])
    assert a.ensemble_families == 4 and parse(["options", "out", "--ensemble", "16", "--ensemble-families", "6"]).ensemble_families == 6
    assert parse(["options", "out", "--ensemble", "16"]).ensemble_families is None
    for argv in (["options", "out", "--ensemble-families"], ["options", "out", "--ensemble", "16", "--ensemble-families", "9"]):
        with pytest.raises(SystemExit):
            parse(argv)
