"""CPU tier: the FDEM forward, Jacobian and misfit against a long-double evaluation of the reference's formula.

``oracle/libgbp_oracle_ld.so`` is ``oracle/fdem1d_oracle.c`` with every real a long double (64-bit mantissa on x86).  Against it
this file measures two things on one fixed case set per system: how far the plain fp64 oracle is from the formula's value (that
is the noise the 1e-7 ppm parity bar was sized for) and how far the kernels' numerical scheme (tests/host_emul, the device
headers built by g++) is.  ``scripts/measure_forward_bars.py`` turns the same measurement into
``tests/golden/fdem_ld_bars.json``; the tests here and in ``test_forward_long_double_gpu.py`` hold the scheme / the device to it.

Unit of every bar and ratio: the share of the present parity bar, |x - ld| / (ATOL + RTOL |ld|), with PRED_* for predictions and
Jacobians and LIKE_* for chi^2 and log L (tests/conftest.py).  A cell is (system, altitude band, tensor id, quantity); chi^2 and
log L belong to a sounding, not a channel, and are filed under tensor id 0.
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, LIKE_ATOL, LIKE_RTOL, PRED_ATOL, PRED_RTOL, ROOT, oracle_system

SYSTEMS = ("resolve", "syn10", "mixed")
BANDS = ((0.5, 3.0), (3.0, 30.0), (30.0, 500.0))          # altitude, m
BAND_NAMES = ("0.5-3m", "3-30m", "30-500m")
LAYER_CYCLE = (1, 2, 3, 8, 9, 16, 17, 30)    # half-space, first recursion step, both sides of the (k & 7) == 7 renormalisation, > 8
PER_BAND, N_DEEP, DEEP_LAYERS, N_JAC = 48, 4, 44, 12
SEED = 3          # chosen on the reference side alone: `mixed` below 3 m holds three tid-7 values on which the fp64 oracle leaves the bar
REL_ERR, ADD_ERR = 0.05, 5.0
QUANTITIES = ("pred", "J", "J_exact", "chi2", "logL")
BARS_JSON = os.path.join(GOLDEN, "fdem_ld_bars.json")
U53, U64 = 2.0 ** -53, 2.0 ** -64

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


@functools.lru_cache(maxsize=None)
def _cases(name):
    """One ragged batch per system: 48 soundings per altitude band (log-uniform altitude, layer counts cycling through
    LAYER_CYCLE), then four 44-layer soundings (bands 0, 1, 2, 1); sigma log-uniform 1e-6 .. 1e2 S/m, thickness 0.01 .. 1000 m;
    data as in scripts/stress_parity.py.  ``jac`` lists the soundings whose Jacobian is checked: the first 12 of each band."""
    rng = np.random.default_rng([SEED, SYSTEMS.index(name)])
    B, Lmax = len(BANDS) * PER_BAND + N_DEEP, DEEP_LAYERS
    band = np.r_[np.repeat(np.arange(len(BANDS)), PER_BAND), [0, 1, 2, 1]].astype(np.int32)
    nl = np.r_[np.tile([LAYER_CYCLE[j % len(LAYER_CYCLE)] for j in range(PER_BAND)], len(BANDS)),
               np.full(N_DEEP, DEEP_LAYERS)].astype(np.int32)
    lo, hi = np.array(BANDS)[band].T
    h = np.exp(rng.uniform(np.log(lo), np.log(hi)))
    sig = np.exp(rng.uniform(np.log(1e-6), np.log(1e2), (B, Lmax)))
    thk = np.exp(rng.uniform(np.log(1e-2), np.log(1e3), (B, Lmax)))
    for b in range(B):
        thk[b, nl[b] - 1:] = 0.0             # the last layer is the half-space
    nF = oracle_system(name).nF
    obs = np.abs(rng.normal(size=(B, 2 * nF))) * 100.0
    jac = np.concatenate([np.arange(i * PER_BAND, i * PER_BAND + N_JAC) for i in range(len(BANDS))])
    c = dict(name=name, B=B, Lmax=Lmax, band=band, nl=nl, h=h, sig=sig, thk=thk, obs=obs, jac=jac,
             rel=np.full(B, REL_ERR), add=np.full(B, ADD_ERR))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _jac_sub(c):
    """The Jacobian soundings as a batch of their own, trimmed to their deepest model."""
    j = c["jac"]
    L = int(c["nl"][j].max())
    return c["nl"][j], c["sig"][j, :L], c["thk"][j, :L], c["h"][j]


@functools.lru_cache(maxsize=None)
def long_double_reference(name):
    """Long-double values of the case set, computed once and left unchanged: pred[B, 2F], chi2[B], logL[B] and, for the Jacobian
    soundings, J and J_exact [36, 2F, L]."""
    from oracle import fdem_oracle as fo
    assert fo.mantissa_bits_ld() >= 64
    s, c = oracle_system(name), _cases(name)
    pred, chi2, logl = fo.forward_loglike_batch_ld(s, c["nl"], c["sig"], c["thk"], c["h"], c["obs"], c["rel"], c["add"])
    js = _jac_sub(c)
    r = dict(pred=pred, chi2=chi2, logL=logl, J=fo.sensitivity_batch_ld(s, *js, exact=False),
             J_exact=fo.sensitivity_batch_ld(s, *js, exact=True))
    for v in r.values():
        assert v.dtype == np.longdouble
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_values(name):
    """The plain fp64 oracle on the case set (same keys as ``long_double_reference``)."""
    from oracle import fdem_oracle as fo
    s, c = oracle_system(name), _cases(name)
    pred, chi2, logl = fo.forward_loglike_batch(s, c["nl"], c["sig"], c["thk"], c["h"], c["obs"], c["rel"], c["add"], nthreads=0)
    js = _jac_sub(c)
    out = dict(pred=pred, chi2=chi2, logL=logl)
    try:
        out["J"] = fo.sensitivity_batch(s, *js, nthreads=0)
        fo.set_exact_jacobian(True)
        out["J_exact"] = fo.sensitivity_batch(s, *js, nthreads=0)
    finally:
        fo.set_exact_jacobian(False)
    return out


def _emul_lib():
    d = os.path.join(ROOT, "tests", "host_emul")
    subprocess.check_call(["make", "-s", "-C", d])
    return ctypes.CDLL(os.path.join(d, "libfdem_host_emul.so"))


def _D(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _I(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def scheme_values(name, lib=None):
    """The kernels' scheme on the host (tests/host_emul: emul_fdem_forward, emul_fdem_sens with exact 0 and 1); chi^2 and log L are
    the fp64 misfit of its predictions."""
    from oracle import fdem_oracle as fo
    lib = _emul_lib() if lib is None else lib
    s, c = oracle_system(name), _cases(name)
    keep = [_I(s.tid), _D(s.frequencies), _D(s.tx_xyz[:, 2]), _D(s.rx_xyz[:, 2]), _D(s.tx_moment), _D(s.scale),
            _D(s.rx_off), _D(s.separation), _D(s.w0), _D(s.lamda0), _D(s.w1), _D(s.lamda1)]
    sysp = [q[1] for q in keep]
    pred = np.empty((c["B"], 2 * s.nF))
    a = [_I(c["nl"]), _D(c["sig"]), _D(c["thk"]), _D(c["h"])]
    assert lib.emul_fdem_forward(s.nF, *sysp, c["B"], c["Lmax"], *[q[1] for q in a], pred.ctypes.data_as(_dp)) == 0
    out = dict(pred=pred, chi2=np.empty(c["B"]), logL=np.empty(c["B"]))
    for b in range(c["B"]):
        _, out["chi2"][b], out["logL"][b], _ = fo.gauss_loglike(pred[b], c["obs"][b], REL_ERR, ADD_ERR)
    nl, sig, thk, h = _jac_sub(c)
    a = [_I(nl), _D(sig), _D(thk), _D(h)]
    for key, exact in (("J", 0), ("J_exact", 1)):
        J = np.empty((nl.size, 2 * s.nF, sig.shape[1]))
        assert lib.emul_fdem_sens(s.nF, *sysp, nl.size, sig.shape[1], *[q[1] for q in a], exact, J.ctypes.data_as(_dp)) == 0
        out[key] = J
    return out


def present_bar(quantity, ref):
    ref = np.abs(np.asarray(ref, dtype=np.longdouble))
    if quantity in ("chi2", "logL"):
        return LIKE_ATOL + LIKE_RTOL * ref
    return PRED_ATOL + PRED_RTOL * ref


def cell_key(name, band, tid, quantity):
    return "%s/%s/tid%d/%s" % (name, BAND_NAMES[band], tid, quantity)


def cells(name, quantity):
    """(key, boolean mask over the quantity's array) for every cell of one system and quantity."""
    s, c = oracle_system(name), _cases(name)
    ref = long_double_reference(name)[quantity]
    rows = c["band"] if quantity in ("pred", "chi2", "logL") else c["band"][c["jac"]]
    out = []
    for bi in range(len(BANDS)):
        if quantity in ("chi2", "logL"):
            out.append((cell_key(name, bi, 0, quantity), rows == bi))
            continue
        for t in sorted(set(int(x) for x in s.tid)):
            chan = np.tile(s.tid == t, 2)                      # [Re block, Im block]
            m = np.zeros(ref.shape, dtype=bool)
            m[np.ix_(rows == bi, chan)] = True
            out.append((cell_key(name, bi, t, quantity), m))
    return out


def ratios(quantity, x, ref):
    """|x - ld| / present bar, element-wise, in long double; a non-finite value anywhere is an error, never dropped."""
    x = np.asarray(x)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    d = np.abs(x.astype(np.longdouble) - ref)
    assert np.all(np.isfinite(d)), "non-finite value in " + quantity
    return d / present_bar(quantity, ref)


def measure(name, scheme=None):
    """{cell: {"oracle": largest ratio of the fp64 oracle, "scheme": of the host emulation, "oracle_abs", "scheme_abs": the largest
    absolute distances}} over every cell of one system."""
    ref, orc = long_double_reference(name), oracle_values(name)
    sch = scheme_values(name) if scheme is None else scheme
    out = {}
    for q in QUANTITIES:
        ro, rs = ratios(q, orc[q], ref[q]), ratios(q, sch[q], ref[q])
        bar = present_bar(q, ref[q])
        for key, m in cells(name, q):
            out[key] = dict(oracle=float(ro[m].max()), scheme=float(rs[m].max()),
                            oracle_abs=float((ro * bar)[m].max()), scheme_abs=float((rs * bar)[m].max()))
    return out


def bars_from(meas):
    """reference_bar: the fp64 oracle's largest distance in the cell, at most the present bar (1).  scheme_bar: four times the
    emulation's, at most reference_bar and at least 16 * 2^-11 of the oracle's distance (the long-double value's own rounding,
    from the ratio of the unit round-offs)."""
    out = {}
    for key, m in meas.items():
        rb = min(m["oracle"], 1.0)
        sb = min(max(4.0 * m["scheme"], 16.0 * 2.0 ** -11 * m["oracle"]), rb)
        out[key] = dict(reference_bar=rb, scheme_bar=sb, oracle_abs=m["oracle_abs"], scheme_abs=m["scheme_abs"])
    return out


@functools.lru_cache(maxsize=None)
def load_bars():
    with open(BARS_JSON) as f:
        return json.load(f)["cells"]


def worst(name, quantity, r, m):
    """Where the largest ratio of a cell sits: 'sounding 17 (L 3, h 1.2 m) row 4 [layer 2]'."""
    c = _cases(name)
    i = np.unravel_index(int(np.argmax(np.where(m, r, -1.0))), r.shape)
    b = int(i[0]) if quantity in ("pred", "chi2", "logL") else int(c["jac"][i[0]])
    txt = "sounding %d (L %d, h %.3g m)" % (b, c["nl"][b], c["h"][b])
    if len(i) > 1:
        txt += " row %d" % i[1]
    if len(i) > 2:
        txt += " layer %d" % i[2]
    return txt


def hold(name, quantity, x, which, extra=0.0, what="", ref=None):
    """Assert every cell of one quantity within its bar (``which``: reference_bar or scheme_bar; ``extra``: an absolute allowance
    on top, in the quantity's own unit).  Returns the largest ratio to the bar."""
    ref = long_double_reference(name)[quantity] if ref is None else ref
    r = ratios(quantity, x, ref)
    bars, top, bad = load_bars(), 0.0, []
    for key, m in cells(name, quantity):
        allowed = bars[key][which] + extra / present_bar(quantity, ref)
        rel = r / allowed
        top = max(top, float(rel[m].max()))
        if rel[m].max() > 1.0:
            bad.append("%s %s: %s, ratio to %s %.3g" % (what, key, worst(name, quantity, rel, m), which, float(rel[m].max())))
    assert not bad, "\n".join(bad)
    return top


@pytest.fixture(scope="module")
def emul():
    return _emul_lib()


@pytest.fixture(scope="module")
def scheme(emul):
    return {n: scheme_values(n, emul) for n in SYSTEMS}


def test_long_double_library_is_wider_than_fp64_and_its_values_are_finite():
    from oracle import fdem_oracle as fo
    assert fo.mantissa_bits_ld() >= 64
    for name in SYSTEMS:
        for k, v in long_double_reference(name).items():
            assert v.dtype == np.longdouble and np.all(np.isfinite(v)), (name, k)
        c = _cases(name)
        assert c["B"] == 148 and sorted(set(c["nl"])) == sorted(LAYER_CYCLE + (DEEP_LAYERS,))
        for bi, (lo, hi) in enumerate(BANDS):
            assert np.all((c["h"][c["band"] == bi] >= lo) & (c["h"][c["band"] == bi] <= hi))


def test_committed_bars_are_what_the_measurement_gives(scheme):
    """tests/golden/fdem_ld_bars.json against a fresh measurement: every bar within 2 % or an absolute 1e-6 of the share (libm and
    compiler versions move the last digits), and the conditions that are not measurements."""
    bars = load_bars()
    fresh = {}
    for name in SYSTEMS:
        fresh.update(bars_from(measure(name, scheme[name])))
    assert set(fresh) == set(bars)
    for key, b in bars.items():
        assert b["scheme_bar"] <= b["reference_bar"] <= 1.0, key
        for w in ("reference_bar", "scheme_bar"):
            assert abs(fresh[key][w] - b[w]) <= 0.02 * b[w] + 1e-6, (key, w, fresh[key][w], b[w])
        if key.endswith("/pred") and "/0.5-3m/" not in key:
            assert b["scheme_bar"] <= 0.1, key           # above 3 m the scheme is held at least ten times tighter than before


@pytest.mark.parametrize("name", SYSTEMS)
def test_oracle_and_scheme_against_long_double(scheme, name):
    """(a) reference_bar is the fp64 oracle's own distance from long double (test_committed_bars_...); the scheme meets it (it is
    at least as accurate as a plain fp64 evaluation of the reference's formula) and scheme_bar (regression pin), in every cell and
    quantity."""
    for q in QUANTITIES:
        hold(name, q, scheme[name][q], "reference_bar", what="scheme")
        hold(name, q, scheme[name][q], "scheme_bar", what="scheme")


def test_mixed_low_altitude_outlier_is_the_oracle_not_the_scheme(scheme):
    """on `mixed` below 3 m, Tx-x/Rx-z channel (tensor id 7), the fp64 evaluation of the reference's H - H0
    is outside the parity bar of the formula's own value and the kernel's scheme is inside it."""
    name = "mixed"
    ref = long_double_reference(name)["pred"]
    m = dict(cells(name, "pred"))[cell_key(name, 0, 7, "pred")]
    ro = ratios("pred", oracle_values(name)["pred"], ref)
    rs = ratios("pred", scheme[name]["pred"], ref)
    print("mixed 0.5-3 m tid 7: oracle %.3g, scheme %.3g of the bar; %d of %d values of the oracle outside"
          % (ro[m].max(), rs[m].max(), int((ro[m] > 1.0).sum()), int(m.sum())))
    assert (ro[m] > 1.0).any(), "the case set holds no sounding on which the fp64 oracle leaves the bar"
    assert np.all(rs[m] <= 1.0), worst(name, "pred", rs, m)


FD_STEP = 2.0 ** -5


def richardson_fd(system, nl, sig, thk, height):
    """d pred / d ln sigma_m of the long-double forward for a batch of soundings, and what that quotient itself may be off by.

    Central differences D(h), D(h/2), D(h/4) with h = 2^-5 (the step actually taken is ln of the ratio of the fp64 conductivities
    the solve sees), extrapolated twice: R1(h) = (4 D(h/2) - D(h)) / 3, R2 = (16 R1(h/2) - R1(h)) / 15, truncation O(h^6).
    Allowance = |R2 - R1(h/2)|, the correction the last extrapolation made and so a bound of what is left of it while the sequence
    converges, plus the rounding of the long-double predictions through the quotient: a long-double prediction is taken to be
    2^-11 of what an fp64 one is off by (the ratio of the unit round-offs), an fp64 one at most four present bars (the largest
    measured is 2.3), and the quotient and the extrapolation weights multiply it by (1 / (h/4)) (16 * 4 / 3 + 16 / 3 + 4 / 3 + 1 / 3) / 15.
    Returns (fd, allowance), both [B, 2F, Lmax] long double, zero beyond a sounding's layers."""
    from oracle import fdem_oracle as fo
    nl, sig, thk, height = np.asarray(nl), np.asarray(sig), np.asarray(thk), np.asarray(height)
    idx = [(r, m) for r in range(nl.size) for m in range(nl[r])]
    n, mm = len(idx), np.array([m for _, m in idx])
    rr = np.tile([r for r, _ in idx], 6)
    steps = (FD_STEP, -FD_STEP, FD_STEP / 2, -FD_STEP / 2, FD_STEP / 4, -FD_STEP / 4)
    batch_sig = sig[rr].copy()
    for k, step in enumerate(steps):
        batch_sig[k * n + np.arange(n), mm] *= np.exp(step)
    p, _, _ = fo.forward_loglike_batch_ld(system, nl[rr], batch_sig, thk[rr], height[rr])
    base = sig[rr[:n], mm].astype(np.longdouble)
    taken = [np.log(batch_sig[k * n + np.arange(n), mm].astype(np.longdouble) / base) for k in range(6)]
    D = [(p[2 * k * n:(2 * k + 1) * n] - p[(2 * k + 1) * n:(2 * k + 2) * n]) / (taken[2 * k] - taken[2 * k + 1])[:, None]
         for k in range(3)]
    R1a, R1b = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
    R2 = (16.0 * R1b - R1a) / 15.0
    p0, _, _ = fo.forward_loglike_batch_ld(system, nl, sig, thk, height)
    noise = 4.0 * 2.0 ** -11 * present_bar("pred", p0)[rr[:n]] / (FD_STEP / 4) * ((64 + 16 + 4 + 1) / 3.0) / 15.0
    fd = np.zeros((nl.size, p.shape[1], sig.shape[1]), dtype=np.longdouble)
    allow = np.zeros_like(fd)
    for k, (r, m) in enumerate(idx):
        fd[r, :, m] = R2[k]
        allow[r, :, m] = np.abs(R2[k] - R1b[k]) + noise[k]
    return fd, allow


@pytest.mark.parametrize("name", SYSTEMS)
def test_exact_jacobian_in_long_double_is_the_derivative_of_the_forward_solve(scheme, name):
    """(b) Validates the reference itself: the long-double exact Jacobian against Richardson-extrapolated central differences of
    the long-double forward in ln sigma, for all 36 Jacobian soundings; then the scheme's exact Jacobian against the long-double
    one."""
    c = _cases(name)
    Jx = long_double_reference(name)["J_exact"]
    fd, allow = richardson_fd(oracle_system(name), *_jac_sub(c))
    live = np.arange(fd.shape[2])[None, None, :] < c["nl"][c["jac"]][:, None, None]
    live = np.broadcast_to(live, fd.shape)
    err = np.abs(Jx - fd)
    print(name, "largest |J_exact_ld - fd| / allowance %.3g; largest allowance / present bar %.3g; largest |J_exact_ld - fd| %.3g"
          % (float((err[live] / allow[live]).max()), float((allow / present_bar("J", Jx))[live].max()), float(err.max())))
    assert np.all(err[live] <= allow[live]), (name, float((err[live] / allow[live]).max()))
    assert np.all(Jx[~live] == 0.0)
    # the reference's own expression is NOT that derivative above the half-space: the quotient tells them apart
    Jr = long_double_reference(name)["J"]
    assert np.any(np.abs(Jr - fd)[live] > 1e3 * allow[live])
    hold(name, "J_exact", scheme[name]["J_exact"], "scheme_bar", what="scheme")


@pytest.mark.parametrize("name", SYSTEMS)
def test_gaussian_misfit_fp64_against_long_double(name):
    """(c) oracle_gauss_loglike in fp64 against its long-double build on the same fp64 predictions and data: the distance is the
    rounding of 2F terms, each a few unit round-offs: (2F + 8) u of the sum of the magnitudes added."""
    from oracle import fdem_oracle as fo
    c, pred = _cases(name), oracle_values(name)["pred"]
    N = pred.shape[1]
    for b in range(c["B"]):
        sd, chi2, logl, na = fo.gauss_loglike(pred[b], c["obs"][b], REL_ERR, ADD_ERR)
        sdl, chi2l, logll, nal = fo.gauss_loglike_ld(pred[b], c["obs"][b], REL_ERR, ADD_ERR)
        assert na == nal == N and sdl.dtype == np.longdouble
        assert np.all(np.abs(sd - sdl) <= 2 * U53 * sdl)
        assert abs(chi2 - chi2l) <= (N + 8) * U53 * chi2l, (name, b)
        mag = 0.5 * chi2l + 0.5 * np.sum(np.abs(np.log(sdl * sdl))) + 0.5 * N * np.log(2 * np.pi)
        assert abs(logl - logll) <= (N + 8) * U53 * mag, (name, b)
