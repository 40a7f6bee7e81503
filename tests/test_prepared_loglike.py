"""Fused likelihood from prepared terms (gbp_gauss_prepare + gbp_fdem_forward_loglike_prepared_ex, what FdemBatch.forward_loglike
launches) against the plain entry gbp_fdem_forward_loglike_ex on the same device arrays: the raw bytes of chi2, logL and pred are
equal, for every row, NaN rows and untouched rows included.  The CPU tier checks that header, bindings and wrapper agree."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SENTINEL = -7.0


# ---------------------------------------------------------------------------------------------- CPU tier
def _prototype(hdr, name):
    m = re.search(r"gbp_status\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), hdr, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_bindings_and_wrapper_agree():
    from geobipy_amd import _lib
    from geobipy_amd.batch import FdemBatch
    hdr = open(os.path.join(ROOT, "include", "geobipy_amd.h")).read()
    plain = {"gbp_fdem_forward_loglike": "gbp_fdem_forward_loglike_prepared",
             "gbp_fdem_forward_loglike_ex": "gbp_fdem_forward_loglike_prepared_ex",
             "gbp_bench_time_forward_loglike": "gbp_bench_time_forward_loglike_prepared"}
    for old, new in plain.items():
        a, b = _prototype(hdr, old), _prototype(hdr, new)
        # the prepared entry differs from the plain one in two arguments only: weight, c0 in place of rel, add
        assert len(a) == len(b)
        assert [x for x, y in zip(a, b) if x != y] == ["const double *rel", "const double *add"]
        assert [y for x, y in zip(a, b) if x != y] == ["const double *weight", "const double *c0"]
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
    args = _prototype(hdr, "gbp_gauss_prepare")
    assert [a.split()[-1].lstrip("*") for a in args] == ["B", "N", "obs", "rel", "add", "weight", "c0", "stream"]
    res, argtypes = _lib.SIGNATURES["gbp_gauss_prepare"]
    assert res is _lib.c_int and len(argtypes) == len(args) and argtypes[:2] == [_lib.c_int, _lib.c_int]
    for attr in ("_prepared", "invalidate_prepared", "forward_loglike", "time_forward_loglike"):
        assert callable(getattr(FdemBatch, attr))


def test_library_exports_the_prepared_entries():
    import ctypes
    from geobipy_amd import _lib
    from geobipy_amd.build import build_native
    build_native()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gbp_gauss_prepare", "gbp_fdem_forward_loglike_prepared", "gbp_fdem_forward_loglike_prepared_ex",
                 "gbp_bench_time_forward_loglike_prepared", "gbp_fdem_forward_loglike_ex"):
        assert hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------- GPU tier
def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b))


def _run_both(fb, want_pred):
    """(prepared, plain): chi2, logL, pred of FdemBatch.forward_loglike and of gbp_fdem_forward_loglike_ex called directly on the
    batch's own device arrays; every output is filled with a sentinel first, so rows a kernel leaves alone compare as well."""
    import torch
    from geobipy_amd import _lib
    for t in (fb.chi2, fb.logL, fb.predicted):
        t.fill_(SENTINEL)
    c, l = fb.forward_loglike(want_pred=want_pred)
    got = (c.clone(), l.clone(), fb.predicted.clone())
    ref = tuple(torch.full_like(t, SENTINEL) for t in got)
    with torch.cuda.device(fb.device):
        _lib.check(_lib.load().gbp_fdem_forward_loglike_ex(
            fb._h.ptr, fb.B, fb.Lmax, fb.nlayers.data_ptr(), fb.sigma.data_ptr(), fb.thk.data_ptr(), fb.height.data_ptr(),
            fb.data.data_ptr(), fb.relative_error.data_ptr(), fb.additive_error.data_ptr(),
            ref[2].data_ptr() if want_pred else None, ref[0].data_ptr(), ref[1].data_ptr(), fb.waves,
            torch.cuda.current_stream(fb.device).cuda_stream))
    torch.cuda.synchronize()
    return got, ref


def _assert_equal(fb, want_pred, what):
    got, ref = _run_both(fb, want_pred)
    for name, a, b in zip(("chi2", "logL", "pred"), got, ref):
        assert _same_bits(a, b), (what, name, int((_bytes(a).reshape(a.shape[0], -1) != _bytes(b).reshape(b.shape[0], -1)).any(1).sum()))
    return got


def _headline_batch(B, waves, eps=None, special=False):
    """Rows of the benchmark's batch (10 frequencies x 8 layers, observed = forward(true model) + 5 % + 5 ppm noise, fresh proposal
    conductivities).  `special` adds the rows the likelihood defines case by case."""
    from geobipy_amd import FdemBatch, synthetic
    s = synthetic.syn10_system()
    nl, sig_true, thk, h = synthetic.draw_models(B, 8, seed=synthetic.SEED + 2)
    clean = FdemBatch(s, nl, sig_true, thk, h).forward().cpu().numpy()
    obs = synthetic.noisy_observations(clean, seed=synthetic.SEED + 3)
    sig = synthetic.redraw_sigma(B, 8, seed=synthetic.SEED + 10)
    rel, add = np.full(B, 0.05), np.full(B, 5.0)
    nl = nl.copy()
    if special:
        rng = np.random.default_rng(5)
        rel, add = rng.uniform(0.01, 0.2, B), rng.uniform(0.5, 20.0, B)
        obs[10, 3] = 0.0                       # data <= 0: inactive
        obs[11, [0, 7, 19]] = -12.5
        obs[12, 5] = np.nan                    # NaN data: inactive
        obs[13, :] = np.nan                    # no active channel
        obs[14, :] = -1.0
        obs[15, :] = 0.0
        obs[16, 4] = np.inf                    # active, infinite variance
        add[17] = 0.0
        rel[18], add[18] = 0.0, 0.0            # zero variance: infinite weight
        rel[19] = np.nan
        nl[20] = 0                             # skipped: outputs untouched
        nl[21] = 9                             # more layers than Lmax = 8: NaNs
        nl[22] = 1000000
        sig[23, 2] = -1.0                      # a bad conductivity: whatever it gives, both entries give it
        sig[24, 0] = np.nan                    # non-finite prediction poisons chi2
        nl[25:40] = rng.integers(1, 9, 15)     # ragged layer counts
        sig[40, :] = 1e-7                      # below sigma_direct: the general complex square root
    fb = FdemBatch(s, nl, sig, thk, h, data=obs, relative_error=rel, additive_error=add, waves=waves, hankel_eps_ppm=eps)
    if special:                                # altitudes outside the batch's bins, set after the handle was built for the others
        fb.height[30] = 0.5                    # below the first altitude bin: the handle's own tables, all abscissae
        fb.height[31] = float(fb.height.min().item()) - 3.0
        fb.height[32] = float("nan")
        fb.height[33] = 5000.0                 # above the last bin
    return fb


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4, 16, 0])
@pytest.mark.parametrize("want_pred", [False, True])
def test_headline_rows(waves, want_pred):
    B = 9000 if waves == 0 else 3000           # waves = 0 from 8 192 rows up: the library picks one wave per sounding
    _assert_equal(_headline_batch(B, waves), want_pred, ("headline", waves))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("eps", [None, 0.0])
def test_special_rows(waves, eps):
    """Inactive channels, NaN data, no active channel, degenerate error levels, skipped and oversized rows, non-finite predictions,
    altitudes below the first bin / NaN / above the last bin; with the default windows and with all abscissae (eps = 0: the general
    passes, frequencies that straddle a pass)."""
    import torch
    for want_pred in (False, True):
        fb = _headline_batch(2048, waves, eps=eps, special=True)
        chi2, logL, pred = _assert_equal(fb, want_pred, ("special", waves, eps))
        assert (chi2[[13, 14, 15]] == 0).all() and (logL[[13, 14, 15]] == 0).all()
        assert chi2[20] == SENTINEL and logL[20] == SENTINEL and (pred[20] == SENTINEL).all()
        assert torch.isnan(chi2[[21, 22, 24]]).all() and torch.isnan(logL[[21, 22, 24]]).all()
        assert torch.isfinite(chi2[[10, 11, 12, 30, 31, 33, 40]]).all()
        if want_pred:
            assert torch.isnan(pred[[21, 22]]).all()
        else:
            assert (pred == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4, 16])
def test_mixed_system_ragged_layers(waves):
    """The `mixed` system (every tensor id) with L = 1, 8, 9, 30 in one ragged batch of Lmax = 32."""
    from geobipy_amd import FdemBatch, FdemSystem, synthetic
    s = FdemSystem.read(os.path.join(GOLDEN, "mixed.stm"))
    parts = [synthetic.draw_models(300, L, seed=100 + L, Lmax=32) for L in (1, 8, 9, 30)]
    nl, sig, thk, h = (np.concatenate([p[i] for p in parts]) for i in range(4))
    clean = FdemBatch(s, nl, sig, thk, h).forward().cpu().numpy()
    obs = synthetic.noisy_observations(clean, seed=7)
    prop = np.concatenate([synthetic.redraw_sigma(300, L, seed=200 + L, Lmax=32) for L in (1, 8, 9, 30)])
    rng = np.random.default_rng(9)
    B = nl.size
    for eps in (None, 0.0):
        fb = FdemBatch(s, nl, prop, thk, h, data=obs, relative_error=rng.uniform(0.02, 0.1, B), additive_error=rng.uniform(1.0, 9.0, B),
                       waves=waves, hankel_eps_ppm=eps)
        for want_pred in (False, True):
            _assert_equal(fb, want_pred, ("mixed", waves, eps))


@pytest.mark.gpu
def test_prepared_terms_follow_their_inputs():
    """Two calls without an edit prepare once; an in-place edit or a replacement of data, relative_error or additive_error prepares
    again, and the result is that of a freshly built batch, bit for bit."""
    import torch
    from geobipy_amd import FdemBatch, synthetic
    s = synthetic.syn10_system()
    B = 512
    nl, sig, thk, h = synthetic.draw_models(B, 5, seed=77)
    clean = FdemBatch(s, nl, sig, thk, h).forward().cpu().numpy()
    obs = synthetic.noisy_observations(clean, seed=78)
    prop = synthetic.redraw_sigma(B, 5, seed=79)
    fb = FdemBatch(s, nl, prop, thk, h, data=obs, relative_error=np.full(B, 0.05), additive_error=np.full(B, 5.0))

    def fresh():
        f = FdemBatch(s, nl, prop, thk, h, data=fb.data.clone(), relative_error=fb.relative_error.clone(),
                      additive_error=fb.additive_error.clone())
        c, l = f.forward_loglike()
        assert f.n_prepare_launches == 1
        return c.clone(), l.clone(), f.predicted.clone()

    def check(expected_launches, what):
        c, l = fb.forward_loglike()
        assert fb.n_prepare_launches == expected_launches, what
        for a, b in zip((c, l, fb.predicted), fresh()):
            assert _same_bits(a, b), what
        _assert_equal(fb, True, what)                      # (one more forward_loglike, no edit in between)
        assert fb.n_prepare_launches == expected_launches, what
        return c.clone(), l.clone()

    assert fb.n_prepare_launches == 0
    c0, l0 = check(1, "first use")
    fb.forward_loglike(want_pred=False)
    fb.time_forward_loglike(2)
    assert fb.n_prepare_launches == 1
    n = 1
    edits = [("data in place", lambda: fb.data.mul_(1.07)),
             ("one datum in place", lambda: fb.data.__setitem__((3, 2), -1.0)),
             ("relative_error in place", lambda: fb.relative_error.fill_(0.08)),
             ("additive_error in place", lambda: fb.additive_error.add_(1.5)),
             ("data replaced", lambda: setattr(fb, "data", fb.data * 0.9)),
             ("relative_error replaced", lambda: setattr(fb, "relative_error", torch.full_like(fb.relative_error, 0.03))),
             ("additive_error replaced", lambda: setattr(fb, "additive_error", fb.additive_error * 2.0))]
    prev = (c0, l0)
    for what, edit in edits:
        edit()
        n += 1
        cur = check(n, what)
        assert not _same_bits(cur[1], prev[1]), what       # the edit is visible in logL, so a stale cache would have been caught
        prev = cur
    fb.invalidate_prepared()
    check(n + 1, "explicit invalidation")
