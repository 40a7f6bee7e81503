"""Posterior ensembles, host side (CPU tier): the run-length arithmetic of the store against the per-iteration loop, the raster's rule
in numpy against plain loops, the argument checks and the block size with an ensemble in the payload budget."""
import numpy as np
import pytest

from geobipy_amd import inference, survey_run
from geobipy_amd.inference import Posteriors, ensemble_argument, ensemble_slots


def _loop(dwells, thin, n_keep):
    """The obvious loop: every iteration is one sample; sample n is kept iff n % thin == 0 and n // thin < n_keep, in slot n // thin.
    Returns the model index (position in ``dwells``) every slot holds, -1 for an empty slot."""
    slots = np.full(n_keep, -1)
    n = 0
    for m, d in enumerate(dwells):
        for _ in range(d):
            if n % thin == 0 and n // thin < n_keep:
                slots[n // thin] = m
            n += 1
    return slots, n


def _run_lengths(dwells, thin, n_keep):
    slots = np.full(n_keep, -1)
    seen = 0
    for m, d in enumerate(dwells):
        r = ensemble_slots(seen, d, thin, n_keep)
        assert all(slots[s] == -1 for s in r)                     # a slot is written once
        slots[list(r)] = m
        seen += d
    return slots, seen


@pytest.mark.parametrize("thin, n_keep, max_dwell", [(3, 64, 10), (1, 40, 5), (7, 16, 30), (2, 40, 4), (5, 1, 9), (4, 4096, 3), (1, 1, 1)])
def test_ensemble_slots_equal_the_per_iteration_loop(thin, n_keep, max_dwell):
    rng = np.random.default_rng(thin * 1000 + n_keep)
    for _ in range(20):
        dwells = rng.integers(0, max_dwell + 1, size=int(rng.integers(1, 60)))      # d = 0 among them
        a, na = _loop(dwells, thin, n_keep)
        b, nb = _run_lengths(dwells, thin, n_keep)
        assert np.array_equal(a, b) and na == nb == dwells.sum()
        filled = min(n_keep, -(-na // thin))
        assert (b >= 0).sum() == filled and np.all(b[:filled] >= 0) and np.all(np.diff(b[:filled]) >= 0)      # chain order, no holes


def test_ensemble_slots_edge_cases():
    assert list(ensemble_slots(0, 0, 3, 8)) == []                 # d = 0 writes nothing, not even slot 0
    assert list(ensemble_slots(6, 0, 3, 8)) == []
    assert list(ensemble_slots(0, 1, 3, 8)) == [0]
    assert list(ensemble_slots(6, 1, 3, 8)) == [2]                # seen an exact multiple of thin: the settle's first sample is kept
    assert list(ensemble_slots(7, 2, 3, 8)) == []                 # samples 7, 8: none kept
    assert list(ensemble_slots(7, 3, 3, 8)) == [3]
    assert list(ensemble_slots(4, 20, 3, 8)) == [2, 3, 4, 5, 6, 7]       # dwell > thin: one model in several slots
    assert list(ensemble_slots(5, 100, 1, 8)) == [5, 6, 7]       # thin = 1, the cap reached in the middle of a dwell
    assert list(ensemble_slots(8, 100, 1, 8)) == []               # past the last slot: dropped, no ring
    assert list(ensemble_slots(1000, 5, 2, 8)) == []
    for bad in ((-1, 1, 1, 1), (0, -1, 1, 1), (0, 1, 0, 1), (0, 1, 1, 0)):
        with pytest.raises(ValueError):
            ensemble_slots(*bad)


def test_host_posteriors_record_per_iteration():
    rng = np.random.default_rng(5)
    K, thin, n_keep = 6, 3, 5
    p = Posteriors(K, 150.0, 1.0, 0.01, ensemble=dict(n_keep=n_keep, thin=thin))
    models = []
    for it in range(11):
        k = int(rng.integers(1, K + 1))
        e, s = np.sort(rng.uniform(1.0, 140.0, k - 1)), rng.uniform(1e-3, 1.0, k)
        models.append((k, e, s, float(it)))
        p.update(e, s, misfit=float(it))
    assert p.ens_seen == 11 and np.array_equal(p.ens_k > 0, [True, True, True, True, False])
    for slot in range(4):
        k, e, s, m = models[slot * thin]
        assert p.ens_k[slot] == k and p.ens_misfit[slot] == m
        assert np.array_equal(p.ens_edges[slot, :k - 1], e) and np.all(np.isposinf(p.ens_edges[slot, k - 1:]))
        assert np.array_equal(p.ens_sigma[slot, :k], s) and np.all(np.isnan(p.ens_sigma[slot, k:]))
    p.reset()
    assert p.ens_seen == 0 and not p.ens_k.any()
    off = Posteriors(K, 150.0, 1.0, 0.01)
    off.update(np.zeros(0), np.array([0.01]))
    assert off.ens_k.size == 0 and off.ens_seen == 0


def test_realisations_reference_against_plain_loops():
    from geobipy_amd.ensembles import realisations_reference
    rng = np.random.default_rng(9)
    B, n_keep, K = 3, 4, 7
    k = rng.integers(0, K + 1, (B, n_keep))
    k[0, 0], k[1, 1] = 0, K
    edges, sigma = np.full((B, n_keep, K), np.inf), np.full((B, n_keep, K), np.nan)
    depth_edges = np.linspace(0.0, 100.0, 26)
    z = 0.5 * (depth_edges[:-1] + depth_edges[1:])
    for b in range(B):
        for s in range(n_keep):
            e = np.sort(rng.uniform(0.0, 110.0, max(k[b, s] - 1, 0)))
            if e.size:
                e[0] = z[3]                                       # an interface exactly at a cell centre
            edges[b, s, :e.size] = np.sort(e)
            sigma[b, s, :k[b, s]] = rng.uniform(1e-3, 1.0, k[b, s])
    slots = [2, 0, 0, 3]
    got = realisations_reference(k, edges, sigma, depth_edges, slots)
    assert got.shape == (B, 4, 25)
    for b in range(B):
        for r, s in enumerate(slots):
            for c in range(25):
                if k[b, s] == 0:
                    assert np.isnan(got[b, r, c])
                    continue
                layer = sum(1 for l in range(k[b, s] - 1) if edges[b, s, l] <= z[c])
                assert got[b, r, c] == sigma[b, s, layer]
    assert np.array_equal(realisations_reference(k, edges, sigma, depth_edges)[:, 2], got[:, 0], equal_nan=True)      # slots=None: all, in order


def test_arguments_are_checked():
    from geobipy_amd import _lib, ensembles
    assert ensemble_argument(None) is None and ensemble_argument(False) is None
    assert ensemble_argument(16, n_markov_chains=100, reference_schedule=True) == dict(n_keep=16, thin=7)
    assert ensemble_argument(dict(thin=None), n_markov_chains=100000, reference_schedule=True) == dict(n_keep=256, thin=391)
    assert ensemble_argument(dict(n_keep=40, thin=2)) == dict(n_keep=40, thin=2)
    for bad in (0, 4097, -1, 2.5, True, dict(n_keep=8, thin=0), dict(n_keep=8, thin=1.5), dict(n_keep=8, thin=1, ring=True)):
        with pytest.raises(ValueError):
            ensemble_argument(bad, n_markov_chains=100, reference_schedule=True)
    with pytest.raises(ValueError, match="thin"):
        ensemble_argument(16)                                     # no schedule: thin is required
    with pytest.raises(ValueError, match="thin"):
        ensemble_argument(dict(n_keep=16), n_markov_chains=100, reference_schedule=False)
    with pytest.raises(ValueError):
        inference.check_ensemble(4097, 1)
    assert np.array_equal(ensembles.check_slots(None, 3), [0, 1, 2]) and np.array_equal(ensembles.check_slots([2, 0, 2], 3), [2, 0, 2])
    for bad in ([3], [-1], [], [0.5], [[0]]):
        with pytest.raises(ValueError):
            ensembles.check_slots(bad, 3)
    assert ensembles.depth_axis((12, 0.5)) == (12, 0.5) and ensembles.depth_axis(np.arange(5) * 2.0) == (4, 2.0)
    for bad in ((0, 1.0), (4, 0.0), (4, float("nan")), [1.0, 2.0, 3.0], [0.0, 1.0, 3.0], [0.0]):
        with pytest.raises(ValueError):
            ensembles.depth_axis(bad)
    with pytest.raises(ValueError):
        ensembles.centres([0.0, 2.0, 1.0])
    # host tensors are refused: there is no fallback
    torch = pytest.importorskip("torch")
    ens = ensembles.Ensemble(torch.ones((2, 3), dtype=torch.int32), torch.full((2, 3, 4), float("inf"), dtype=torch.float64),
                             torch.ones((2, 3, 4), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.float64),
                             torch.full((2,), 3), 1, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(_lib.NativeLibraryError):
        ensembles.realisations(ens, [0.0, 1.0, 2.0])
    with pytest.raises(_lib.NativeLibraryError):
        ensembles.rebin(ens, 20, 2.0, (8, 1.0))


def test_save_and_load_round_trip(tmp_path):
    from geobipy_amd import ensembles
    rng = np.random.default_rng(2)
    ens = ensembles.Ensemble(rng.integers(0, 4, (2, 3)).astype(np.int32), rng.uniform(size=(2, 3, 4)), rng.uniform(size=(2, 3, 4)),
                             rng.uniform(size=(2, 3)), np.array([3, 2]), 5, rng.uniform(size=2))
    back = ensembles.load(ensembles.save(ens, str(tmp_path / "ens.npz")))
    assert back.thin == 5 and all(np.array_equal(a, b) for a, b in zip(ens, back))


def test_default_block_counts_the_ensemble():
    assert survey_run.ensemble_bytes(256, 30) == 256 * (16 * 30 + 12) + 4 == 125956      # 126 KB beside the hit map's 440 KB
    for args in ((100000, 1, True, 1), (100000, None, False, 1), (5000, 25, True, 4), (100000, None, True, 2)):
        assert survey_run.default_block(*args) == survey_run.default_block(*args, ensemble_bytes=0)       # unchanged at 0
    per = survey_run.ensemble_bytes(4096, 30)
    assert survey_run.default_block(100000, None, False, 1) == 16384
    assert survey_run.default_block(100000, None, False, 1, ensemble_bytes=per) == (8 << 30) // per < 16384
    with_map = survey_run.default_block(100000, None, True, 1)
    assert survey_run.default_block(100000, None, True, 1, ensemble_bytes=per) == (8 << 30) // (per + 440 * 1024) < with_map
    assert survey_run.default_block(100000, None, True, 2, ensemble_bytes=per) == (8 << 30) // (2 * (per + 440 * 1024))
    assert "ensemble" in survey_run.PHASES


def test_command_line_default():
    from geobipy_amd.__main__ import parse
    assert parse(["options", "out"]).ensemble is None
    assert parse(["options", "out", "--ensemble"]).ensemble == dict(n_keep=64, thin=None)
    assert parse(["options", "out", "--ensemble", "32", "5"]).ensemble == dict(n_keep=32, thin=5)
    for bad in (["--ensemble", "0"], ["--ensemble", "8", "0"], ["--ensemble", "8", "2", "3"], ["--ensemble", "--no-hitmap"]):
        with pytest.raises(SystemExit):
            parse(["options", "out"] + bad)
