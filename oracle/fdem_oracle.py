"""ctypes front-end of oracle/fdem1d_oracle.c (TEST INFRASTRUCTURE, not product code).

Restates, on the CPU in scalar fp64, the reference path
``FdemDataPoint.forward -> fdem1dfwd -> nbFdem1dfwd`` (+ ``nbFdem1dsen``) and
``DataPoint.data_misfit / likelihood`` -- see the C file for the line-by-line citations.
Parity pin: tests/test_oracle_golden.py checks it against fixtures dumped from the imported
reference and against the reference's own ``tests/data_checks/resolve_*_clean.csv``.
"""
import ctypes
import os
import subprocess

import numpy as np

from .gs_filters import W0_J0_120, W1_J1_140, base_abscissae

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def build(force=False):
    """Compile libgbp_oracle.so with gcc (oracle/Makefile)."""
    so = os.path.join(_HERE, "libgbp_oracle.so")
    src = os.path.join(_HERE, "fdem1d_oracle.c")
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", _HERE, "-B", "libgbp_oracle.so"])
    return so


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libgbp_oracle.so")
        if not os.path.exists(so):
            build()
        _LIB = ctypes.CDLL(so)
        _LIB.oracle_fdem1dfwd.restype = ctypes.c_int
        _LIB.oracle_fdem1dsen.restype = ctypes.c_int
        _LIB.oracle_fdem_forward_loglike_batch.restype = ctypes.c_int
        _LIB.oracle_gauss_loglike.restype = None
        _LIB.oracle_set_exact_jacobian.restype = None
    return _LIB


def set_exact_jacobian(exact):
    """Test switch: ``sensitivity`` returns the true derivative of the forward recursion instead of the reference's M1_1
    expression (which is not one).  Process-wide; the CPU replays of exact-Jacobian device chains set it."""
    lib().oracle_set_exact_jacobian(ctypes.c_int(1 if exact else 0))


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


class OracleSystem:
    """Plain-array stand-in for the tables of ``FdemSystem`` (system/FdemSystem.py:52-109,199-203).

    orientation letters follow EmLoop.py:168-181 (x, y, z = 0, 1, 2);
    tensor_id = 1 + 3*rx_orient + tx_orient.
    """

    _ORI = {"x": 0, "y": 1, "z": 2}

    def __init__(self, frequencies, tx_orient, tx_moment, tx_xyz, rx_orient, rx_moment, rx_xyz):
        self.frequencies = np.asarray(frequencies, dtype=np.float64)
        F = self.frequencies.size
        to = np.array([self._ORI[str(o).strip()] for o in tx_orient], dtype=np.int32)
        ro = np.array([self._ORI[str(o).strip()] for o in rx_orient], dtype=np.int32)
        self.tid = (1 + ro * 3 + to).astype(np.int32)
        self.tx_moment = np.asarray(tx_moment, dtype=np.float64)
        self.rx_moment = np.asarray(rx_moment, dtype=np.float64)
        self.tx_xyz = np.asarray(tx_xyz, dtype=np.float64).reshape(F, 3)
        self.rx_xyz = np.asarray(rx_xyz, dtype=np.float64).reshape(F, 3)
        off = self.rx_xyz - self.tx_xyz                      # FdemSystem.py:52-57
        self.rx_off = np.ascontiguousarray(off[:, 0])        # fdem1d.py:34
        self.separation = np.linalg.norm(off.T, axis=0)      # FdemSystem.py:59-61
        self.scale = self.tx_moment * self.rx_moment         # fdem1d.py:33
        l0, l1 = base_abscissae()
        r = 1.0 / self.separation
        self.lamda0 = np.ascontiguousarray(l0[None, :] * r[:, None])   # FdemSystem.py:67-83
        self.lamda1 = np.ascontiguousarray(l1[None, :] * r[:, None])   # FdemSystem.py:85-101
        self.lamda02 = self.lamda0 ** 2.0
        self.lamda12 = self.lamda1 ** 2.0
        self.w0 = W0_J0_120
        self.w1 = W1_J1_140

    @property
    def nF(self):
        return self.frequencies.size

    @classmethod
    def read(cls, filename):
        """Parse a .stm FDEM system file (FdemSystem.py:146-183): header + one CSV row per frequency."""
        rows = []
        with open(filename) as f:
            next(f)
            for line in f:
                p = [x.strip() for x in line.split(",")]
                if len(p) >= 11:
                    rows.append(p)
        fr = [float(p[0]) for p in rows]
        return cls(fr, [p[1] for p in rows], [float(p[2]) for p in rows],
                   [[float(p[3]), float(p[4]), float(p[5])] for p in rows],
                   [p[6] for p in rows], [float(p[7]) for p in rows],
                   [[float(p[8]), float(p[9]), float(p[10])] for p in rows])


def _sysargs(s, height):
    tH = height + s.tx_xyz[:, 2]            # fdem1d.py:31
    rH = -tH + s.rx_xyz[:, 2]               # fdem1d.py:32
    return tH, rH


def forward(system, conductivity, thickness, height):
    """nbFdem1dfwd for one sounding -> complex128[F]."""
    s = system
    sig, psig = _d(conductivity)
    L = sig.size
    thk, pthk = _d(thickness)
    assert thk.size == L
    zeros, pz = _d(np.zeros(L))
    tH, rH = _sysargs(s, float(height))
    out = np.empty(2 * s.nF)
    keep = [_i(s.tid), _d(s.frequencies), _d(tH), _d(rH), _d(s.tx_moment), _d(s.rx_off), _d(s.separation),
            _d(s.w0), _d(s.lamda0), _d(s.lamda02), _d(s.w1), _d(s.lamda1), _d(s.lamda12), _d(s.scale)]
    rc = lib().oracle_fdem1dfwd(ctypes.c_int(s.nF), ctypes.c_int(L), *[k[1] for k in keep],
                                psig, pz, pz, pthk, out.ctypes.data_as(_dp))
    if rc != 0:
        raise ValueError("unsupported tensor id in system (reference leaves H undefined)")
    return out[0::2] + 1j * out[1::2]


def sensitivity(system, conductivity, thickness, height):
    """nbFdem1dsen for one sounding -> complex128[F, L] (d/dln sigma_k, ppm)."""
    s = system
    sig, psig = _d(conductivity)
    L = sig.size
    thk, pthk = _d(thickness)
    zeros, pz = _d(np.zeros(L))
    tH, rH = _sysargs(s, float(height))
    out = np.empty(2 * s.nF * L)
    keep = [_i(s.tid), _d(s.frequencies), _d(tH), _d(rH), _d(s.tx_moment), _d(s.rx_off), _d(s.separation),
            _d(s.w0), _d(s.lamda0), _d(s.lamda02), _d(s.w1), _d(s.lamda1), _d(s.lamda12), _d(s.scale)]
    rc = lib().oracle_fdem1dsen(ctypes.c_int(s.nF), ctypes.c_int(L), *[k[1] for k in keep],
                                psig, pz, pz, pthk, out.ctypes.data_as(_dp))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    return (out[0::2] + 1j * out[1::2]).reshape(s.nF, L)


def predicted_data(system, conductivity, thickness, height):
    """FdemDataPoint._forward1D layout: [Re(out), Im(out)] (FdemDataPoint.py:544-545)."""
    c = forward(system, conductivity, thickness, height)
    return np.concatenate([c.real, c.imag])


def gauss_loglike(pred, obs, rel, add):
    """(std[N], chi2, logL, n_active) -- DataPoint.py:268-282, 491-525; MvNormalDistribution.py:201-216."""
    p, pp = _d(pred)
    o, po = _d(obs)
    N = p.size
    sd = np.empty(N)
    chi2 = ctypes.c_double()
    logl = ctypes.c_double()
    na = ctypes.c_int()
    lib().oracle_gauss_loglike(ctypes.c_int(N), pp, po, ctypes.c_double(rel), ctypes.c_double(add),
                               sd.ctypes.data_as(_dp), ctypes.byref(chi2), ctypes.byref(logl), ctypes.byref(na))
    return sd, chi2.value, logl.value, na.value


def _sysargs_batch(s, conv):
    return [_i(s.tid), conv(s.frequencies), conv(s.tx_xyz[:, 2]), conv(s.rx_xyz[:, 2]), conv(s.tx_moment), conv(s.scale),
            conv(s.rx_off), conv(s.separation)]


def sensitivity_batch(system, nlayers, sigma, thk, height, nthreads=1):
    """Batched fp64 Jacobian J[B, 2F, Lmax] (rows [Re, Im], zero beyond a sounding's layers); mode as ``set_exact_jacobian``."""
    s = system
    nl, pnl = _i(nlayers)
    sig, psig = _d(sigma)
    B, Lmax = sig.shape
    th, pth = _d(thk)
    h, ph = _d(height)
    assert s.nF <= 64 and nl.size == B and th.shape == sig.shape and h.size == B
    J = np.empty((B, 2 * s.nF, Lmax))
    keep = _sysargs_batch(s, _d) + [_d(s.w0), _d(s.lamda0), _d(s.lamda02), _d(s.w1), _d(s.lamda1), _d(s.lamda12)]
    rc = lib().oracle_fdem_sens_batch(ctypes.c_int(B), ctypes.c_int(s.nF), ctypes.c_int(Lmax), *[k[1] for k in keep],
                                      pnl, psig, pth, ph, J.ctypes.data_as(_dp), ctypes.c_int(nthreads))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    return J


# ---- the long-double build (libgbp_oracle_ld.so): the same C file with every real a long double -------------------------
# Inputs are the fp64 values the fp64 oracle and the kernels see (frequencies, geometry, lamda, weights, sigma, thickness,
# height; tHeight / rHeight are formed in fp64 as fdem1d.py does) widened exactly; lamda^2 is formed here in long double.
# Outputs are np.longdouble.  Every converted array stays referenced by a local until the ctypes call has returned.
_LIB_LD = None
MAX_THREADS_LD = 16


def lib_ld():
    global _LIB_LD
    if _LIB_LD is None:
        so = os.path.join(_HERE, "libgbp_oracle_ld.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-s", "-C", _HERE, "-B", "libgbp_oracle_ld.so"])
        L = ctypes.CDLL(so)
        L.oracle_real_mant_dig.restype = ctypes.c_int
        for f in ("oracle_fdem1dfwd", "oracle_fdem1dsen", "oracle_fdem_forward_loglike_batch", "oracle_fdem_sens_batch"):
            getattr(L, f).restype = ctypes.c_int
        L.oracle_gauss_loglike.restype = None
        L.oracle_set_exact_jacobian.restype = None
        # the C long double must be numpy's longdouble, and wider than fp64 by the 11 bits the bars reason with
        assert L.oracle_real_mant_dig() >= 64, "long double has a %d-bit mantissa, 64 needed" % L.oracle_real_mant_dig()
        assert np.finfo(np.longdouble).nmant + 1 == L.oracle_real_mant_dig() and \
            np.dtype(np.longdouble).itemsize == ctypes.sizeof(ctypes.c_longdouble)
        _LIB_LD = L
    return _LIB_LD


def mantissa_bits_ld():
    """LDBL_MANT_DIG of the long-double library (64 on x86)."""
    return lib_ld().oracle_real_mant_dig()


def _q(a):
    a = np.ascontiguousarray(a, dtype=np.longdouble)
    return a, ctypes.c_void_p(a.ctypes.data)


def _threads_ld(nthreads):
    n = int(nthreads)
    if n <= 0:
        n = os.cpu_count() or 1
    return max(1, min(n, MAX_THREADS_LD))


def _tables_ld(s):
    l0, l1 = np.asarray(s.lamda0, dtype=np.longdouble), np.asarray(s.lamda1, dtype=np.longdouble)
    return [_q(s.w0), _q(l0), _q(l0 * l0), _q(s.w1), _q(l1), _q(l1 * l1)]


def _one_ld(fn, system, conductivity, thickness, height, nout):
    s = system
    sig, psig = _q(conductivity)
    L = sig.size
    thk, pthk = _q(thickness)
    assert thk.size == L
    zeros, pz = _q(np.zeros(L))
    tH, rH = _sysargs(s, float(height))          # fp64, as the fp64 oracle forms them
    out = np.empty(2 * nout(L), dtype=np.longdouble)
    keep = [_i(s.tid), _q(s.frequencies), _q(tH), _q(rH), _q(s.tx_moment), _q(s.rx_off), _q(s.separation)] + \
        _tables_ld(s) + [_q(s.scale)]
    rc = fn(ctypes.c_int(s.nF), ctypes.c_int(L), *[k[1] for k in keep], psig, pz, pz, pthk, ctypes.c_void_p(out.ctypes.data))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    del keep, sig, thk, zeros
    return out[0::2] + 1j * out[1::2]


def forward_ld(system, conductivity, thickness, height):
    """``forward`` in long double -> clongdouble[F]."""
    return _one_ld(lib_ld().oracle_fdem1dfwd, system, conductivity, thickness, height, lambda L: system.nF)


def sensitivity_ld(system, conductivity, thickness, height, exact=False):
    """``sensitivity`` in long double -> clongdouble[F, L]; ``exact``: the true derivative of the forward recursion."""
    L = np.size(conductivity)
    lib_ld().oracle_set_exact_jacobian(ctypes.c_int(1 if exact else 0))
    try:
        return _one_ld(lib_ld().oracle_fdem1dsen, system, conductivity, thickness, height,
                       lambda L: system.nF * L).reshape(system.nF, L)
    finally:
        lib_ld().oracle_set_exact_jacobian(ctypes.c_int(0))


def gauss_loglike_ld(pred, obs, rel, add):
    """``gauss_loglike`` in long double: (std[N], chi2, logL, n_active), the first three np.longdouble."""
    p, pp = _q(pred)
    o, po = _q(obs)
    N = p.size
    sd = np.empty(N, dtype=np.longdouble)
    res = np.empty(2, dtype=np.longdouble)
    na = ctypes.c_int()
    ra = ctypes.c_longdouble(np.float64(rel))
    lib_ld().oracle_gauss_loglike(ctypes.c_int(N), pp, po, ra, ctypes.c_longdouble(np.float64(add)),
                                  ctypes.c_void_p(sd.ctypes.data), ctypes.c_void_p(res.ctypes.data),
                                  ctypes.c_void_p(res.ctypes.data + res.itemsize), ctypes.byref(na))
    del p, o
    return sd, res[0], res[1], na.value


def forward_loglike_batch_ld(system, nlayers, sigma, thk, height, obs=None, rel=None, add=None, nthreads=0):
    """``forward_loglike_batch`` in long double (OpenMP over soundings, at most 16 threads): pred[B, 2F], chi2[B], logL[B]
    as np.longdouble.  ``obs`` may be fp64 or long double (predictions of this build, say)."""
    s = system
    nl, pnl = _i(nlayers)
    B = nl.size
    sig, psig = _q(sigma)
    Lmax = sig.shape[1]
    th, pth = _q(thk)
    h, ph = _q(height)
    assert s.nF <= 64 and th.shape == sig.shape and h.size == B
    pred = np.empty((B, 2 * s.nF), dtype=np.longdouble)
    chi2 = np.full(B, np.nan, dtype=np.longdouble)
    logl = np.full(B, np.nan, dtype=np.longdouble)
    if obs is not None:
        o, po = _q(obs)
        r, pr = _q(np.broadcast_to(rel, (B,)))
        a, pa = _q(np.broadcast_to(add, (B,)))
    else:
        o = r = a = po = pr = pa = None
    keep = _sysargs_batch(s, _q) + _tables_ld(s)
    rc = lib_ld().oracle_fdem_forward_loglike_batch(
        ctypes.c_int(B), ctypes.c_int(s.nF), ctypes.c_int(Lmax), *[k[1] for k in keep], pnl, psig, pth, ph,
        po, pr, pa, ctypes.c_void_p(pred.ctypes.data), ctypes.c_void_p(chi2.ctypes.data),
        ctypes.c_void_p(logl.ctypes.data), ctypes.c_int(_threads_ld(nthreads)))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    del keep, sig, th, h, o, r, a
    return pred, chi2, logl


def sensitivity_batch_ld(system, nlayers, sigma, thk, height, exact=False, nthreads=0):
    """``sensitivity_batch`` in long double -> np.longdouble J[B, 2F, Lmax]."""
    s = system
    nl, pnl = _i(nlayers)
    sig, psig = _q(sigma)
    B, Lmax = sig.shape
    th, pth = _q(thk)
    h, ph = _q(height)
    assert s.nF <= 64 and nl.size == B and th.shape == sig.shape and h.size == B
    J = np.empty((B, 2 * s.nF, Lmax), dtype=np.longdouble)
    keep = _sysargs_batch(s, _q) + _tables_ld(s)
    lib_ld().oracle_set_exact_jacobian(ctypes.c_int(1 if exact else 0))
    try:
        rc = lib_ld().oracle_fdem_sens_batch(ctypes.c_int(B), ctypes.c_int(s.nF), ctypes.c_int(Lmax),
                                             *[k[1] for k in keep], pnl, psig, pth, ph, ctypes.c_void_p(J.ctypes.data),
                                             ctypes.c_int(_threads_ld(nthreads)))
    finally:
        lib_ld().oracle_set_exact_jacobian(ctypes.c_int(0))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    del keep, sig, th, h
    return J


def forward_loglike_batch(system, nlayers, sigma, thk, height, obs=None, rel=None, add=None, nthreads=1):
    """Batched oracle (and the "port" CPU baseline of bench.py): returns pred[B,2F], chi2[B], logL[B]."""
    s = system
    nl, pnl = _i(nlayers)
    B = nl.size
    sig, psig = _d(sigma)
    Lmax = sig.shape[1]
    th, pth = _d(thk)
    h, ph = _d(height)
    assert s.nF <= 64
    pred = np.empty((B, 2 * s.nF))
    chi2 = np.full(B, np.nan)
    logl = np.full(B, np.nan)
    if obs is not None:
        o, po = _d(obs)
        r, pr = _d(np.broadcast_to(rel, (B,)))
        a, pa = _d(np.broadcast_to(add, (B,)))
    else:
        po = pr = pa = None
    keep = [_i(s.tid), _d(s.frequencies), _d(s.tx_xyz[:, 2]), _d(s.rx_xyz[:, 2]), _d(s.tx_moment), _d(s.scale),
            _d(s.rx_off), _d(s.separation), _d(s.w0), _d(s.lamda0), _d(s.lamda02), _d(s.w1), _d(s.lamda1),
            _d(s.lamda12)]
    rc = lib().oracle_fdem_forward_loglike_batch(
        ctypes.c_int(B), ctypes.c_int(s.nF), ctypes.c_int(Lmax), *[k[1] for k in keep], pnl, psig, pth, ph,
        po, pr, pa, pred.ctypes.data_as(_dp), chi2.ctypes.data_as(_dp), logl.ctypes.data_as(_dp),
        ctypes.c_int(nthreads))
    if rc != 0:
        raise ValueError("unsupported tensor id in system")
    return pred, chi2, logl
