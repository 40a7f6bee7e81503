"""The forward kernel's outputs, bit for bit, at every model depth from 1 to 34 layers.

forward_passes_1f walks a sounding's layers in pieces whose seams depend on the depth: the step above the basement is peeled, the
layers below 8 are an unrolled chain entered at the sounding's own depth, deeper models reach the chain's top through a loop, and the
renormalisation falls on k = 7, 15, 23, 31.  tests/test_forward_bits.py pins L = 1, 7, 8, 9, 30; this file pins every L from 1 to 34, for
the `syn10` system windowed (forward_passes_1f) and with all abscissae (the general forward_passes), with 1 and 4 waves per sounding.
tests/golden/forward_layer_digests.json holds, per case, the SHA-256 of the float64 predictions of FdemBatch.forward() and of
(chi2, logL) of forward_loglike(want_pred=False), recorded by tests/golden/make_forward_layer_digests.py with the library of the commit
before the layer records of forward_passes_1f.
"""
import hashlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "forward_layer_digests.json")
MODES = ("windowed", "all")
WAVES = (1, 4)
LAYERS = tuple(range(1, 35))
B = 48


def _models(L):
    """The draw of test_forward_bits._models: altitudes over 2 .. 120 m, every fifth row with a 1e-6 S/m layer (non-DIRECT branch)."""
    from geobipy_amd import synthetic
    nl, sigma, thk, height = synthetic.draw_models(B, L, seed=synthetic.SEED + L)
    rng = np.random.default_rng(1000 + L)
    height = rng.uniform(2.0, 120.0, size=B)
    sigma[::5, min(1, L - 1)] = 1e-6
    return nl, sigma, thk, height


def _data(L, F):
    """Seeded positive data and error levels for the likelihood."""
    rng = np.random.default_rng(2000 + L)
    return rng.uniform(20.0, 400.0, size=(B, 2 * F)), np.full(B, 0.05), np.full(B, 5.0)


def _cases():
    for m in MODES:
        for w in WAVES:
            for L in LAYERS:
                yield "syn10_%s_w%d_L%d" % (m, w, L), m, w, L


def _batch(system, mode, waves, L, sigma=None):
    from geobipy_amd import FdemBatch
    nl, sig, thk, height = _models(L)
    data, rel, add = _data(L, system.nFrequencies)
    return FdemBatch(system, nl, sig if sigma is None else sigma, thk, height, data=data, relative_error=rel, additive_error=add,
                     hankel_eps_ppm=(0.0 if mode == "all" else None), waves=waves)


def outputs(system, mode, waves, L):
    """(pred [B, 2F], like [2, B]) of one case: FdemBatch.forward() and (chi2, logL) of forward_loglike(want_pred=False)."""
    import torch
    fb = _batch(system, mode, waves, L)
    pred = fb.forward()
    chi2, logL = fb.forward_loglike(want_pred=False)
    torch.cuda.synchronize()
    to_np = lambda t: np.ascontiguousarray(t.cpu().numpy().astype(np.float64, copy=False))
    return to_np(pred), np.stack([to_np(chi2), to_np(logL)])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def record():
    """{case: {"pred": sha256, "like": sha256}} of every case with the library loaded in this process."""
    from geobipy_amd import synthetic
    system = synthetic.syn10_system()
    rec = {}
    for key, m, w, L in _cases():
        pred, like = outputs(system, m, w, L)
        assert np.isfinite(pred).all() and np.isfinite(like).all(), key
        rec[key] = {"pred": digest(pred), "like": digest(like)}
    return rec


def test_layer_digest_record_covers_every_case():
    with open(DIGESTS) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(k for k, *_ in _cases())
    assert len(rec) == len(MODES) * len(WAVES) * len(LAYERS)
    assert all(sorted(v) == ["like", "pred"] and all(len(d) == 64 for d in v.values()) for v in rec.values())


@pytest.mark.gpu
def test_forward_outputs_bit_identical_at_every_depth():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    from geobipy_amd import synthetic
    with open(DIGESTS) as f:
        rec = json.load(f)
    system = synthetic.syn10_system()
    bad = []
    by_case = {}
    for key, m, w, L in _cases():
        pred, like = outputs(system, m, w, L)
        assert np.isfinite(pred).all() and np.isfinite(like).all(), key
        by_case[key] = (pred, like)
        if digest(pred) != rec[key]["pred"]:
            bad.append(key + ":pred")
        if digest(like) != rec[key]["like"]:
            bad.append(key + ":like")
    assert not bad, "outputs differ from the recorded bits: %s" % ", ".join(bad)
    # the number of waves per sounding never changes a bit
    for m in MODES:
        for L in LAYERS:
            p1, l1 = by_case["syn10_%s_w1_L%d" % (m, L)]
            p4, l4 = by_case["syn10_%s_w4_L%d" % (m, L)]
            assert np.array_equal(p1, p4) and np.array_equal(l1, l4), (m, L)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("L", (2, 8, 11))
def test_nan_sigma_row_is_nan_and_leaves_its_neighbours_alone(L, waves):
    """A row with a NaN conductivity returns NaN chi2 / logL (and predictions); every other row keeps its bits."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    from geobipy_amd import synthetic
    system = synthetic.syn10_system()
    _, ref = outputs(system, "windowed", waves, L)
    _, sigma, _, _ = _models(L)
    rows = (3, 17, B - 1)                       # (none of them a 1e-6 S/m row: those are rows 0, 5, 10, ...)
    for i, r in enumerate(rows):
        sigma[r, (L - 1, 0, L // 2)[i]] = np.nan   # basement, top layer, a layer between
    fb = _batch(system, "windowed", waves, L, sigma=sigma)
    pred = fb.forward().cpu().numpy()
    chi2, logL = fb.forward_loglike(want_pred=False)
    torch.cuda.synchronize()
    like = np.stack([chi2.cpu().numpy(), logL.cpu().numpy()])
    keep = np.ones(B, dtype=bool)
    keep[list(rows)] = False
    assert np.isnan(like[:, ~keep]).all()
    assert np.isnan(pred[~keep]).all()
    assert np.array_equal(like[:, keep], ref[:, keep])
