"""GPU tier: the FDEM kernels against the long-double oracle, held to the bars of tests/golden/fdem_ld_bars.json.

Same case set as tests/test_forward_long_double.py (148 ragged soundings per system); the long-double values are computed on the
host at test time from oracle/libgbp_oracle_ld.so.  ``scheme_bar`` is four times the distance of the kernels' scheme on the host
(tests/host_emul) from long double, capped by ``reference_bar``, the fp64 oracle's own distance -- so a kernel that loses a term
of its exponential, or a renormalisation of its recursion, fails here while it is still far inside the 1e-7 ppm parity bar.
Launch shapes: the ragged batch of 148 with waves = 1 and the default, and the same soundings one at a time (B = 1).
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_forward_long_double import (SYSTEMS, _cases, _jac_sub, hold, long_double_reference)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def _system(name):
    from geobipy_amd import FdemSystem
    return FdemSystem.read(os.path.join(GOLDEN, name + ".stm"))


def _batch(name, rows=None, **kw):
    from geobipy_amd import FdemBatch
    c = _cases(name)
    rows = slice(None) if rows is None else rows
    w = lambda k: np.array(c[k][rows])          # the shared case arrays are read-only; torch wants writable memory
    return FdemBatch(_system(name), w("nl"), w("sig"), w("thk"), w("h"), data=w("obs"), relative_error=w("rel"),
                     additive_error=w("add"), **kw)


def _jbatch(name, **kw):
    from geobipy_amd import FdemBatch
    return FdemBatch(_system(name), *(np.array(a) for a in _jac_sub(_cases(name))), hankel_eps_ppm=0.0, **kw)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("waves", [0, 1])
def test_forward_all_abscissae(name, waves):
    top = hold(name, "pred", _np(_batch(name, hankel_eps_ppm=0.0, waves=waves).forward()), "scheme_bar", what="forward waves=%d" % waves)
    print("%s forward waves=%d: largest ratio to scheme_bar %.3g" % (name, waves, top))


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("waves", [0, 1])
def test_forward_default_window(name, waves):
    from geobipy_amd.system import DEFAULT_HANKEL_EPS_PPM
    b = _batch(name, waves=waves)
    assert b.hankel_eps_ppm == DEFAULT_HANKEL_EPS_PPM
    top = hold(name, "pred", _np(b.forward()), "scheme_bar", extra=DEFAULT_HANKEL_EPS_PPM, what="windowed forward waves=%d" % waves)
    print("%s windowed forward waves=%d: largest ratio to scheme_bar + eps %.3g" % (name, waves, top))


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("prepared", [True, False])
@pytest.mark.parametrize("waves", [0, 1])
def test_forward_loglike(name, prepared, waves):
    b = _batch(name, hankel_eps_ppm=0.0, waves=waves)
    chi2, logl = b.forward_loglike(prepared=prepared)
    what = "%s likelihood waves=%d" % ("prepared" if prepared else "fused", waves)
    tops = [hold(name, "pred", _np(b.predicted), "scheme_bar", what=what), hold(name, "chi2", _np(chi2), "scheme_bar", what=what),
            hold(name, "logL", _np(logl), "scheme_bar", what=what)]
    print("%s %s: largest ratio to scheme_bar pred %.3g chi2 %.3g logL %.3g" % (name, what, *tops))


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("exact", [False, True])
def test_sensitivity(name, exact):
    q = "J_exact" if exact else "J"
    top = hold(name, q, _np(_jbatch(name).sensitivity(exact=exact)), "scheme_bar", what="sensitivity")
    print("%s sensitivity exact=%s: largest ratio to scheme_bar %.3g" % (name, exact, top))


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("exact", [False, True])
def test_fm_dlogc_both_outputs(name, exact):
    c = _cases(name)
    b = _jbatch(name)
    J = _np(b.fm_dlogc(exact=exact))
    top = hold(name, "J_exact" if exact else "J", J, "scheme_bar", what="fm_dlogc")
    # its predictions: the Jacobian soundings' rows of the long-double predictions, in a full-size array so that the cells apply
    pred = np.array(long_double_reference(name)["pred"], dtype=np.float64)
    pred[c["jac"]] = _np(b.predicted)
    topp = hold(name, "pred", pred, "scheme_bar", what="fm_dlogc predictions")
    print("%s fm_dlogc exact=%s: largest ratio to scheme_bar J %.3g pred %.3g" % (name, exact, top, topp))


@pytest.mark.parametrize("name", SYSTEMS)
def test_one_sounding_at_a_time(name):
    """B = 1 launches: forward, both likelihood entries and both Jacobian entries for every sounding on its own give what the
    ragged batch is held to."""
    from geobipy_amd import FdemBatch
    c, s = _cases(name), _system(name)
    B, F2 = c["B"], 2 * s.nFrequencies
    pred, predl, chi2, logl, chi2f, loglf = (np.empty((B, F2)), np.empty((B, F2)), np.empty(B), np.empty(B), np.empty(B), np.empty(B))
    jn, js, jh = _jac_sub(c)[0], _jac_sub(c)[1:3], _jac_sub(c)[3]
    J = {k: np.zeros((jn.size, F2, js[0].shape[1])) for k in ("J", "J_exact", "fm")}
    outs = []
    for i in range(B):
        b = _batch(name, rows=slice(i, i + 1), hankel_eps_ppm=0.0)
        outs.append((b.forward().clone(), ) + tuple(t.clone() for t in b.forward_loglike(prepared=True)) + (b.predicted.clone(), )
                    + tuple(t.clone() for t in b.forward_loglike(prepared=False)))
    jouts = []
    for i in range(jn.size):
        L = int(jn[i])
        b = FdemBatch(s, np.array(jn[i:i + 1]), np.array(js[0][i:i + 1, :L]), np.array(js[1][i:i + 1, :L]), np.array(jh[i:i + 1]),
                      hankel_eps_ppm=0.0)
        jouts.append((b.sensitivity(exact=False), b.sensitivity(exact=True), b.fm_dlogc(exact=True)))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        pred[i], chi2[i], logl[i], predl[i], chi2f[i], loglf[i] = (t.cpu().numpy().reshape(-1) if t.numel() > 1 else t.item()
                                                                    for t in o)
    for i, o in enumerate(jouts):
        L = int(jn[i])
        for k, t in zip(("J", "J_exact", "fm"), o):
            J[k][i, :, :L] = t.cpu().numpy()[0]
    tops = [hold(name, "pred", pred, "scheme_bar", what="B=1 forward"), hold(name, "pred", predl, "scheme_bar", what="B=1 likelihood"),
            hold(name, "chi2", chi2, "scheme_bar", what="B=1 prepared"), hold(name, "logL", logl, "scheme_bar", what="B=1 prepared"),
            hold(name, "chi2", chi2f, "scheme_bar", what="B=1 fused"), hold(name, "logL", loglf, "scheme_bar", what="B=1 fused"),
            hold(name, "J", J["J"], "scheme_bar", what="B=1 sensitivity"),
            hold(name, "J_exact", J["J_exact"], "scheme_bar", what="B=1 sensitivity"),
            hold(name, "J_exact", J["fm"], "scheme_bar", what="B=1 fm_dlogc")]
    print("%s one at a time: largest ratios to scheme_bar" % name, " ".join("%.3g" % t for t in tops))


def test_mixed_low_altitude_tid7_on_the_device():
    """The channel on which the fp64 oracle leaves the parity bar of the formula's value (test_forward_long_double.py): the device is
    inside it, and its distance is printed."""
    from test_forward_long_double import cell_key, cells, ratios, present_bar
    name = "mixed"
    ref = long_double_reference(name)["pred"]
    r = ratios("pred", _np(_batch(name, hankel_eps_ppm=0.0).forward()), ref)
    m = dict(cells(name, "pred"))[cell_key(name, 0, 7, "pred")]
    print("mixed 0.5-3 m tid 7 on the device: %.3g of the parity bar, %.3g ppm" % (r[m].max(), (r * present_bar("pred", ref))[m].max()))
    assert np.all(r[m] <= 1.0)
