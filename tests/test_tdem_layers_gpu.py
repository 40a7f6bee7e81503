"""Time-domain kernels over depth, launch shape and the window stage, against references of their own (GPU tier).

Raw Hankel handles have 22 - 110 "frequencies"; the Jacobian kernel's waves per sounding, LDS per wave and row groups per
evaluation depend on that count and on the layer count at once (fm_dlogc_launch), and the window stage (gbp_td_apply_mix) picks
one of three kernels by batch size and LDS need.  Every comparison here is against something the kernels did not produce:
``oracle/tdem_oracle.py`` (numpy, tanh recursion) for the forward and -- by Richardson-extrapolated differences -- the Jacobian,
long double for the window stage and the likelihood alone.  tests/test_tdem_layers.py draws the models and shows on the CPU that
the oracle equals the numpy twin of the device path to 1e-14 of the peak and that the difference reference is stable to 1e-10, so
what is measured here belongs to the kernels.  Measured values: docs/notes_tdem_parity.md.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_tdem_attitude import random_geometry, xyz_system
from test_tdem_layers import JAC_LAYERS, SYSTEMS, draw_model, forward_models, jac_columns, oracle_forward, oracle_richardson, pad_models

pytestmark = pytest.mark.gpu

FILL = -7.0


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _att(g):
    return np.c_[g[:, 1:4], g[:, 7:10]]


def _two_raw_systems(tmp_path):
    """The two raw handles of sections C and D: Tempest in level flight (56 frequencies) and a SkyTEM loop with X / Y / Z outputs
    and attitude (110) -> [(label, path, geometry(B, rng))]."""
    from geobipy_amd.tdem_geometry import gaaem_geometry
    off, alt = SYSTEMS["tempest.stm"]
    return [("tempest level", os.path.join(GOLDEN, "tempest.stm"), 56, lambda B, rng: gaaem_geometry(np.full(B, alt), off)),
            ("skytem xyz attitude", xyz_system("SkytemLM.stm", tmp_path), 110,
             lambda B, rng: random_geometry(rng, B, alt=(25.0, 45.0), rho=(8.0, 110.0)))]


def _oracle_geometry(stm, sig, thk, g):
    from oracle import tdem_oracle as to
    return to.forward_geometry(stm, sig, thk, g)


# ------------------------------------------------------------------------------------------------------------------------
# A. forward, deep and ragged, against the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_forward_deep_and_ragged_against_the_oracle(name):
    """27 soundings of 1 - 44 layers (usual, wide and thin models) in one batch: every row within 1e-8 of its peak of the oracle;
    the same bits with NaN in the unused entries, in another order and with another row stride; all abscissae (hankel_eps = 0) and
    the C-level system meet the same numbers."""
    torch = pytest.importorskip("torch")
    from geobipy_amd.tdem import NativeTdemSystem, TdemBatch, TdemSystem
    from geobipy_amd.tdem_geometry import gaaem_geometry
    path = os.path.join(GOLDEN, name)
    system = TdemSystem(path)
    off, alt = SYSTEMS[name]
    models = [m for _, _, m in forward_models()]
    B = len(models)
    nl, sigma, thk = pad_models(models, 44)
    h = np.full(B, alt)
    out_t = TdemBatch(system, nl, sigma, thk, h, off).forward().clone()
    out = out_t.cpu().numpy()
    assert np.all(np.isfinite(out))
    ref = np.stack([oracle_forward(name, s, t) for s, t in models])
    peak = np.abs(ref).max(axis=1, keepdims=True)
    used = (np.abs(out - ref) / peak).max(axis=1)
    print("A forward vs oracle, %s: used/bar = %.3g (row %d: %d layers)" % (name, used.max() / 1e-8, used.argmax(), nl[used.argmax()]))
    assert np.all(used <= 1e-8), (name, used.argmax(), used.max())
    # poisoned padding
    sp, tp = sigma.copy(), thk.copy()
    for i in range(B):
        sp[i, nl[i]:] = np.nan
        tp[i, nl[i] - 1:] = np.nan
    assert torch.equal(TdemBatch(system, nl, sp, tp, h, off).forward(), out_t)
    # order
    perm = np.random.default_rng(3).permutation(B)
    assert torch.equal(TdemBatch(system, nl[perm], sigma[perm], thk[perm], h, off).forward(), out_t[torch.as_tensor(perm, device=out_t.device)])
    # stride
    nl50, s50, t50 = pad_models(models, 50)
    assert torch.equal(TdemBatch(system, nl50, s50, t50, h, off).forward(), out_t)
    # all abscissae
    full = TdemBatch(system, nl, sigma, thk, h, off, hankel_eps=0.0).forward().cpu().numpy()
    used_full = (np.abs(full - ref) / peak).max()
    used_win = (np.abs(full - out) / peak).max()
    print("A all abscissae, %s: vs oracle used/bar = %.3g, vs default windows used/bar = %.3g" % (name, used_full / 1e-8, used_win / 1e-10))
    assert used_full <= 1e-8 and used_win <= 1e-10
    # the C-level system
    nat = NativeTdemSystem(path).forward(gaaem_geometry(h, off), nl, sigma, thk).cpu().numpy()
    used_nat = (np.abs(nat - out) / peak).max()
    print("A native vs batch, %s: used/bar = %.3g" % (name, used_nat / 1e-10))
    assert used_nat <= 1e-10


# ------------------------------------------------------------------------------------------------------------------------
# B. Jacobian against oracle differences
# ------------------------------------------------------------------------------------------------------------------------
# of the row's peak.  The project's Jacobian bar is 1e-6 (tests/test_tdem.py, kept below for the device's own differences); against
# the oracle the first run measured 5.1e-13 at worst (docs/notes_tdem_parity.md), so this comparison holds the forward's bar, 1e-8
JAC_ORACLE_BAR = 1e-8


@pytest.mark.parametrize("L", JAC_LAYERS)
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_jacobian_against_oracle_differences(name, L):
    """fm_dlogc of two L-layer models: the columns on both sides of every row group against Richardson differences of the oracle,
    all columns against central differences of the device's forward; no column vanishes, the prediction is the forward's, the
    C-level system returns the same Jacobian."""
    torch = pytest.importorskip("torch")
    from geobipy_amd.tdem import NativeTdemSystem, TdemBatch, TdemSystem
    from geobipy_amd.tdem_geometry import gaaem_geometry
    path = os.path.join(GOLDEN, name)
    system = TdemSystem(path)
    off, alt = SYSTEMS[name]
    models = [draw_model("jac", L, seed) for seed in (0, 1)]
    nl, sigma, thk = pad_models(models, L)
    h = np.full(2, alt)
    tb = TdemBatch(system, nl, sigma, thk, h, off)
    fwd = tb.forward().cpu().numpy().copy()
    pred_t, J_t = tb.fm_dlogc()
    pred, J = pred_t.cpu().numpy(), J_t.cpu().numpy()
    assert J.shape == (2, system.n_components * system.nwindows, L) and np.all(np.isfinite(J))
    peak = np.abs(fwd).max(axis=1)
    assert np.all(np.abs(pred - fwd) <= 1e-10 * peak[:, None])
    # against the oracle
    worst, where = 0.0, None
    for b, (sig, th) in enumerate(models):
        f = lambda s: oracle_forward(name, s, th)
        opeak = np.abs(f(sig)).max()
        cache = {}
        for m in jac_columns(L):
            d = np.abs(J[b, :, m] - oracle_richardson(f, sig, m, cache=cache)).max() / opeak
            if d > worst:
                worst, where = d, (b, m)
    print("B Jacobian vs oracle, %s, %d layers: worst |dJ| / peak = %.3e (model %d, column %d), used/bar = %.3g"
          % (name, L, worst, where[0], where[1], worst / JAC_ORACLE_BAR))
    assert worst <= JAC_ORACLE_BAR, (name, L, where, worst)
    # against the device's own forward: all columns, rows (model, column, sign) of one batch
    eps = 1e-4
    sig_fd = np.repeat(sigma, 2 * L, axis=0)
    for b in range(2):
        for m in range(L):
            sig_fd[(b * L + m) * 2, m] *= np.exp(eps)
            sig_fd[(b * L + m) * 2 + 1, m] *= np.exp(-eps)
    f_fd = TdemBatch(system, np.repeat(nl, 2 * L), sig_fd, np.repeat(thk, 2 * L, axis=0), np.full(4 * L, alt), off).forward().cpu().numpy()
    fd = ((f_fd[0::2] - f_fd[1::2]) / (2 * eps)).reshape(2, L, -1).transpose(0, 2, 1)
    assert np.all(np.abs(J - fd) <= 1e-6 * peak[:, None, None]), (name, L, (np.abs(J - fd) / peak[:, None, None]).max())
    # guards and identities
    assert np.all(np.abs(J).max(axis=1) >= 1e-5 * peak[:, None]), (name, L, (np.abs(J).max(axis=1) / peak[:, None]).min())
    assert np.all(J[:, :, L:] == 0.0)
    nl3, s3, t3 = pad_models(models, L + 3)                    # another row stride: the same bits, zeros behind the last layer
    J3 = TdemBatch(system, nl3, s3, t3, h, off).fm_dlogc()[1]
    assert torch.equal(J3[:, :, :L], J_t) and bool((J3[:, :, L:] == 0.0).all())
    pn, Jn = NativeTdemSystem(path).fm_dlogc(gaaem_geometry(h, off), nl, sigma, thk)
    assert np.abs(Jn.cpu().numpy() - J).max() <= 1e-10 * np.abs(J).max() and np.all(np.abs(pn.cpu().numpy() - pred) <= 1e-10 * peak[:, None])


# ------------------------------------------------------------------------------------------------------------------------
# C. ragged Jacobian and max_layers
# ------------------------------------------------------------------------------------------------------------------------
def test_ragged_jacobian_is_the_same_bits_for_every_max_layers(tmp_path):
    """The nodal Jacobian kernel on a batch of all nine layer counts (and skipped rows) with max_layers 8, 16 and 44 -- one, two
    and four row groups per evaluation: rows that fit have the same bits in all three, rows that do not come back NaN, skipped
    rows keep their fill, through the nodal stage and the window stage."""
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib
    from geobipy_amd.tdem import TdemBatch, TdemSystem
    lib = _lib.load()
    counts = [1, 2, 0, 8, 9, 16, 0, 17, 32, 33, 44, 0, 8]
    models = [draw_model("usual", max(L, 1), 5) for L in counts]
    nl, sigma, thk = pad_models(models, 44)
    nl = np.array(counts, dtype=np.int32)
    B = len(counts)
    rng = np.random.default_rng(17)
    for label, path, nF, geometry in _two_raw_systems(tmp_path):
        g = geometry(B, rng)
        tb = TdemBatch(TdemSystem(path), nl, sigma, thk, g[:, 0], g[:, 4:7], attitude=_att(g))
        hnd, mix, W = tb._h[0], tb._mix[0], tb._W[0]
        assert hnd.nF == nF and mix.n_in == 2 * nF
        n_out, N = W.shape
        rows = None if mix.set_of_row is None else mix.set_of_row.data_ptr()
        res = {}
        for ml in (8, 16, 44):
            nodal = torch.full((B, mix.n_in), FILL, dtype=torch.float64, device=tb.device)
            Jn = torch.full((B, mix.n_in, 44), FILL, dtype=torch.float64, device=tb.device)
            _lib.check(lib.gbp_fdem_fm_dlogc_rows_ex(hnd.ptr, B, 44, tb.nlayers.data_ptr(), tb.sigma.data_ptr(), tb.thk.data_ptr(),
                                                     tb.height.data_ptr(), nodal.data_ptr(), Jn.data_ptr(), ml, 1, rows, 0, _stream(torch)))
            pw = torch.full((B, N), FILL, dtype=torch.float64, device=tb.device)
            Jw = torch.full((B, N, 44), FILL, dtype=torch.float64, device=tb.device)
            mx = mix.struct()
            _lib.check(lib.gbp_td_apply_mix(B, 44, n_out, N, tb.nlayers.data_ptr(), W.data_ptr(), nodal.data_ptr(), Jn.data_ptr(),
                                            pw.data_ptr(), Jw.data_ptr(), ctypes.byref(mx), _stream(torch)))
            torch.cuda.synchronize()
            res[ml] = (nodal, Jn, pw, Jw)
        full = res[44]
        for ml in (8, 16, 44):
            nodal, Jn, pw, Jw = res[ml]
            for b, k in enumerate(counts):
                if k == 0:                                            # skipped: the fill survives both stages
                    assert all(bool((x[b] == FILL).all()) for x in (nodal, Jn, pw, Jw)), (label, ml, b)
                elif k > ml:                                          # does not fit this launch: NaN, not an overrun
                    assert bool(torch.isnan(nodal[b]).all()) and bool(torch.isnan(Jn[b]).all()), (label, ml, b)
                    assert bool(torch.isnan(pw[b]).all()) and bool(torch.isnan(Jw[b, :, :k]).all()) and bool((Jw[b, :, k:] == 0.0).all()), (label, ml, b)
                else:                                                 # fits (rows next to NaN and skipped rows among them): same bits
                    assert all(torch.equal(x[b], y[b]) for x, y in zip(res[ml], full)), (label, ml, b, k)
                    assert bool(torch.isfinite(nodal[b]).all()) and bool(torch.isfinite(Jw[b]).all())
                    assert bool((Jn[b, :, k:] == 0.0).all()) and bool((Jw[b, :, k:] == 0.0).all()), (label, ml, b)
                    assert float(Jw[b, :, :k].abs().max()) > 0.0
        # the batch's own entry point runs the max_layers = 44 variant on the rows it evaluates
        live = torch.as_tensor(np.nonzero(nl > 0)[0], device=tb.device)
        pred, J = tb.fm_dlogc()
        assert torch.equal(pred[live], full[2][live]) and torch.equal(J[live], full[3][live])
    # the C-level system sizes its launch by the row stride where the batch takes the deepest model: shallow models in wide rows run
    # the four-group variant there and the one-group variant here
    from geobipy_amd.tdem import NativeTdemSystem
    from geobipy_amd.tdem_geometry import gaaem_geometry
    off, alt = SYSTEMS["tempest.stm"]
    path = os.path.join(GOLDEN, "tempest.stm")
    shallow = [draw_model("usual", L, 7) for L in (1, 2, 5, 8, 8, 3)]
    nl8, s8, t8 = pad_models(shallow, 44)
    h8 = np.full(len(shallow), alt)
    tb = TdemBatch(TdemSystem(path), nl8, s8, t8, h8, off)
    pred, J = tb.fm_dlogc()
    assert tb._max_layers == 8
    pn, Jn = NativeTdemSystem(path).fm_dlogc(gaaem_geometry(h8, off), nl8, s8, t8)
    assert float((Jn - J).abs().max()) <= 1e-10 * float(J.abs().max())
    assert bool(((pn - pred).abs() <= 1e-10 * pred.abs().max(dim=1, keepdim=True).values).all())
    for b, k in enumerate(nl8):
        assert bool((Jn[b, :, k:] == 0.0).all()) and bool((J[b, :, k:] == 0.0).all())


# ------------------------------------------------------------------------------------------------------------------------
# D. launch shape does not change the bits
# ------------------------------------------------------------------------------------------------------------------------
def test_launch_shape_does_not_change_the_bits(tmp_path):
    """32 soundings of 17 layers tiled to 32, 4100 and 8192 rows: many waves per sounding, four, and one (forward); the 150 000 B
    and the 60 000 B LDS caps of the Jacobian launch -- the same bits per sounding; eight rows of the largest launch against the
    oracle."""
    torch = pytest.importorskip("torch")
    from geobipy_amd.tdem import TdemBatch, TdemSystem
    from oracle import tdem_oracle as to
    L = 17
    models = [draw_model("usual", L, seed) for seed in range(32)]
    nl0, sig0, thk0 = pad_models(models, L)
    rng = np.random.default_rng(23)
    for label, path, nF, geometry in _two_raw_systems(tmp_path):
        system, stm = TdemSystem(path), to.parse_stm(path)
        g0 = geometry(32, rng)
        out = {}
        for B in (32, 4100, 8192):
            idx = np.arange(B) % 32
            g = g0[idx]
            tb = TdemBatch(system, nl0[idx], sig0[idx], thk0[idx], g[:, 0], g[:, 4:7], attitude=_att(g))
            assert tb._h[0].nF == nF
            f = tb.forward().clone()
            J = tb.fm_dlogc()[1] if B <= 4100 else None
            out[B] = (idx, f, J)
        base_f, base_J = out[32][1], out[32][2]
        for B in (4100, 8192):
            idx, f, J = out[B]
            it = torch.as_tensor(idx, device=f.device)
            assert torch.equal(f, base_f[it]), (label, B)
            if J is not None:
                assert torch.equal(J, base_J[it]), (label, B)
        idx, f, _ = out[8192]
        f = f.cpu().numpy()
        worst = 0.0
        for row in (0, 13, 31, 1000, 4099, 5000, 8000, 8191):
            sig, th = models[idx[row]]
            ref = _oracle_geometry(stm, sig, th, g0[idx[row]])
            used = np.abs(f[row] - ref).max() / np.abs(ref).max()
            worst = max(worst, used)
            assert used <= 1e-8, (label, row, used)
        print("D one-wave launch (B = 8192) vs oracle, %s: used/bar = %.3g" % (label, worst / 1e-8))


# ------------------------------------------------------------------------------------------------------------------------
# E. LDS border of the window stage
# ------------------------------------------------------------------------------------------------------------------------
def test_window_stage_at_its_lds_border(tmp_path):
    """Three-component Tempest with attitude: 168 nodal values.  With J the window stage stages 168 (K + 1) doubles: K = 43 is
    59 136 B of dynamic LDS -- more than 48 KiB, under the stage's 60 000 B limit -- and must work; K = 44 is refused with a message
    that names the stage, before anything is written."""
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib
    from geobipy_amd.tdem import TdemBatch, TdemSystem
    from oracle import tdem_oracle as to
    path = xyz_system("tempest.stm", tmp_path)
    system, stm = TdemSystem(path), to.parse_stm(path)
    models = [draw_model("jac", 43, 0), draw_model("usual", 43, 0), draw_model("usual", 17, 0), draw_model("usual", 1, 0)]
    B = len(models)
    g = random_geometry(np.random.default_rng(29), B, alt=(90.0, 130.0), rho=(40.0, 120.0))
    nl, sigma, thk = pad_models(models, 43)
    mk = lambda n_, s_, t_, gg: TdemBatch(system, n_, s_, t_, gg[:, 0], gg[:, 4:7], attitude=_att(gg))
    tb = mk(nl, sigma, thk, g)
    assert tb._W[0].shape[0] == 168 and 168 * 44 * 8 == 59136
    pred_t, J_t = tb.fm_dlogc()
    torch.cuda.synchronize()
    pred, J = pred_t.cpu().numpy().copy(), J_t.cpu().numpy()
    fwd = tb.forward().cpu().numpy()
    peak = np.abs(fwd).max(axis=1)
    assert np.all(np.isfinite(J)) and np.all(np.abs(pred - fwd) <= 1e-10 * peak[:, None])
    worst = 0.0
    for b, (sig, th) in enumerate(models):
        ref = _oracle_geometry(stm, sig, th, g[b])
        worst = max(worst, np.abs(fwd[b] - ref).max() / np.abs(ref).max())
    print("E forward vs oracle at K = 43: used/bar = %.3g" % (worst / 1e-8))
    assert worst <= 1e-8
    cols, eps = (0, 16, 32, 42), 1e-4
    rep = 2 * len(cols)
    sig_fd = np.repeat(sigma, rep, axis=0)
    for b in range(B):
        for q, m in enumerate(cols):
            sig_fd[(b * len(cols) + q) * 2, m] *= np.exp(eps)
            sig_fd[(b * len(cols) + q) * 2 + 1, m] *= np.exp(-eps)
    f_fd = mk(np.repeat(nl, rep), sig_fd, np.repeat(thk, rep, axis=0), np.repeat(g, rep, axis=0)).forward().cpu().numpy()
    fd = ((f_fd[0::2] - f_fd[1::2]) / (2 * eps)).reshape(B, len(cols), -1).transpose(0, 2, 1)
    assert np.all(np.abs(J[:, :, list(cols)] - fd) <= 1e-6 * peak[:, None, None]), (np.abs(J[:, :, list(cols)] - fd) / peak[:, None, None]).max()
    assert np.abs(J[0, :, 42]).max() > 0.0 and np.all(J[2, :, 17:] == 0.0) and np.all(J[3, :, 1:] == 0.0)
    # K = 44: 168 * 45 * 8 = 60 480 B
    nl44, s44, t44 = pad_models(models, 44)
    tb44 = mk(nl44, s44, t44, g)
    assert torch.equal(tb44.forward(), tb.forward())                     # (the forward stages the nodal values only)
    tb44.predicted.fill_(FILL)
    with pytest.raises(_lib.NativeLibraryError, match="time-domain stage"):
        tb44.fm_dlogc()
    torch.cuda.synchronize()
    assert bool((tb44.predicted == FILL).all())
    mix, W = tb44._mix[0], tb44._W[0]
    nodal = torch.zeros((B, mix.n_in), dtype=torch.float64, device=tb44.device)
    Jn = torch.zeros((B, mix.n_in, 44), dtype=torch.float64, device=tb44.device)
    pw = torch.full((B, W.shape[1]), FILL, dtype=torch.float64, device=tb44.device)
    Jw = torch.full((B, W.shape[1], 44), FILL, dtype=torch.float64, device=tb44.device)
    mx = mix.struct()
    with pytest.raises(_lib.NativeLibraryError, match="time-domain stage"):
        _lib.check(_lib.load().gbp_td_apply_mix(B, 44, W.shape[0], W.shape[1], tb44.nlayers.data_ptr(), W.data_ptr(), nodal.data_ptr(),
                                                Jn.data_ptr(), pw.data_ptr(), Jw.data_ptr(), ctypes.byref(mx), _stream(torch)))
    torch.cuda.synchronize()
    assert bool((pw == FILL).all()) and bool((Jw == FILL).all())


# ------------------------------------------------------------------------------------------------------------------------
# F. the window stage alone against long double
# ------------------------------------------------------------------------------------------------------------------------
TD_SHAPES = [(1, 1, 2, 1), (63, 6, 44, 19), (64, 6, 44, 19), (65, 6, 112, 30), (79, 9, 112, 30), (130, 3, 56, 70), (70, 5, 168, 45)]


@pytest.mark.parametrize("B,K,n_nodal,N", TD_SHAPES)
def test_td_apply_mix_against_long_double(B, K, n_nodal, N):
    """gbp_td_apply_mix on random W, nodal values and nodal Jacobians, ragged layer counts with skipped rows among them: without
    and with a synthetic three-term mix (some terms unused), without and with an offset, with J (k_td_apply<true>) and without (B <
    64 or a window operator too large for LDS: k_td_apply<false>; otherwise k_td_apply_plain).  Every output within
    (n_nodal + terms + 4) 2^-52 sum |terms| of the long-double value -- n_nodal + terms roundings of 2^-53 each would be the
    worst case of the sums, so the bound has a factor two and four roundings to spare --, zeros behind a row's layers, fills kept,
    and the same prediction bits from all three kernels."""
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib
    lib = _lib.load()
    ld = np.longdouble
    rng = np.random.default_rng([B, K, n_nodal, N])
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev).contiguous()
    nl = rng.integers(0, K + 1, B).astype(np.int32)
    nl[0] = K
    if B > 4:
        nl[1], nl[B // 2], nl[B - 1] = 0, 0, 1
    W = rng.standard_normal((n_nodal, N)) * 10.0 ** rng.uniform(-3, 3, (n_nodal, 1))
    offset = rng.standard_normal((B, N))
    terms, n_in, n_w = 3, n_nodal + 7, 11
    src = rng.integers(0, n_in, (n_nodal, terms)).astype(np.int32)
    src[rng.uniform(size=src.shape) < 0.3] = -1
    src[0] = (-1, 2 % n_in, -1)
    col = rng.integers(0, n_w, (n_nodal, terms)).astype(np.int32)
    weights = rng.standard_normal((B, n_w))
    W_t, nl_t, off_t, src_t, col_t, w_t = up(W), up(nl, torch.int32), up(offset), up(src, torch.int32), up(col, torch.int32), up(weights)

    def launch(rows, nodal_t, Jn_t, with_j, mixed, with_offset):
        pred = torch.full((rows, N), FILL, dtype=torch.float64, device=dev)
        J = torch.full((rows, N, K), FILL, dtype=torch.float64, device=dev) if with_j else None
        mx = _lib.TdMix()
        if mixed:
            mx.n_in, mx.terms, mx.n_weights, mx.src, mx.col, mx.weights = n_in, terms, n_w, src_t.data_ptr(), col_t.data_ptr(), w_t.data_ptr()
        mx.offset = off_t.data_ptr() if with_offset else None
        _lib.check(lib.gbp_td_apply_mix(rows, K, n_nodal, N, nl_t.data_ptr(), W_t.data_ptr(), nodal_t.data_ptr(), Jn_t.data_ptr() if with_j else None,
                                        pred.data_ptr(), J.data_ptr() if with_j else None, ctypes.byref(mx), _stream(torch)))
        torch.cuda.synchronize()
        return pred, J

    live = nl > 0
    for mixed in (False, True):
        width = n_in if mixed else n_nodal
        nodal = rng.standard_normal((B, width)) * 10.0 ** rng.uniform(-2, 2, (B, width))
        Jn = rng.standard_normal((B, width, K)) * 10.0 ** rng.uniform(-2, 2, (B, width, 1))
        nodal_t, Jn_t = up(nodal), up(Jn)
        # long double: staged values and the sum of the magnitudes of everything that is added
        if mixed:
            use = (src >= 0)[None, :, :]
            wt = weights[:, col].astype(ld) * use                                       # [B, n_nodal, terms]
            pick = np.where(src >= 0, src, 0)
            sn_terms = wt * nodal[:, pick].astype(ld)
            sn, sn_mag = sn_terms.sum(axis=2), np.abs(sn_terms).sum(axis=2)
            sj_terms = wt[:, :, :, None] * Jn[:, pick, :].astype(ld)                    # [B, n_nodal, terms, K]
            sj, sj_mag = sj_terms.sum(axis=2), np.abs(sj_terms).sum(axis=2)
        else:
            sn, sn_mag, sj, sj_mag = nodal.astype(ld), np.abs(nodal).astype(ld), Jn.astype(ld), np.abs(Jn).astype(ld)
        Wl = W.astype(ld)
        p_ref, p_mag = sn @ Wl, sn_mag @ np.abs(Wl)
        J_ref = np.einsum("bmk,mg->bgk", sj, Wl)
        J_mag = np.einsum("bmk,mg->bgk", sj_mag, np.abs(Wl))
        factor = ld(n_nodal + (terms if mixed else 0) + 4) * ld(2.0) ** -52
        for with_offset in (False, True):
            pr = p_ref + (offset.astype(ld) if with_offset else 0)
            pm = p_mag + (np.abs(offset).astype(ld) if with_offset else 0)
            pred_j, J = launch(B, nodal_t, Jn_t, True, mixed, with_offset)
            pred_f, _ = launch(B, nodal_t, Jn_t, False, mixed, with_offset)
            assert torch.equal(pred_j, pred_f), (mixed, with_offset)
            p, Jh = pred_j.cpu().numpy(), J.cpu().numpy()
            assert np.all(p[~live] == FILL) and np.all(Jh[~live] == FILL)
            assert np.all(np.isfinite(p[live])) and np.all(np.abs(p[live].astype(ld) - pr[live]) <= factor * pm[live]), (mixed, with_offset)
            for b in np.nonzero(live)[0]:
                k = nl[b]
                assert np.all(np.abs(Jh[b, :, :k].astype(ld) - J_ref[b, :, :k]) <= factor * J_mag[b, :, :k]), (mixed, with_offset, b)
                assert np.all(Jh[b, :, k:] == 0.0), (mixed, with_offset, b)
            if B >= 64:                                                                 # the first 63 rows as a launch of their own
                sub, _ = launch(63, nodal_t, Jn_t, False, mixed, with_offset)
                assert torch.equal(sub, pred_f[:63]), (mixed, with_offset)


# ------------------------------------------------------------------------------------------------------------------------
# G. the likelihood with a standard deviation per channel against long double
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 45, 64, 65, 130])
def test_gauss_loglike_std_against_long_double(N, B):
    """chi^2 = sum ((pred - obs) / sd)^2 and logL = -na/2 ln 2pi - sum ln sd - chi^2 / 2 over the active channels (obs > 0; NaN and
    obs <= 0 are inactive).  Bounds: a term of chi^2 carries seven roundings of 2^-53 (difference, reciprocal and their product,
    twice through the square, and the square's own) and the wave's sum at most 6 + N / 64 more, under (N + 8) 2^-52 for every N;
    logL adds the device logarithm, taken as within 4 * 2^-52 relative as in tests/test_ensemble_correlation_gpu.py."""
    torch = pytest.importorskip("torch")
    from geobipy_amd import _lib
    lib = _lib.load()
    ld = np.longdouble
    rng = np.random.default_rng([N, B])
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev).contiguous()
    obs = 10.0 ** rng.uniform(-13, -9, (B, N))
    pred = obs * (1.0 + 0.1 * rng.standard_normal((B, N)))
    sd = 0.05 * obs * 10.0 ** rng.uniform(-1, 1, (B, N))
    dead = rng.uniform(size=(B, N)) < 0.25
    obs[dead] = rng.choice([0.0, -1e-11, np.nan], size=int(dead.sum()))
    cases = [obs]
    gone = obs.copy()
    gone[B // 2] = rng.choice([0.0, -1e-11, np.nan], size=N)       # a row with every channel inactive
    cases.append(gone)
    for o in cases:
        chi2 = torch.full((B,), FILL, dtype=torch.float64, device=dev)
        logL = torch.full((B,), FILL, dtype=torch.float64, device=dev)
        p_t, o_t, s_t = up(pred), up(o), up(sd)
        _lib.check(lib.gbp_gauss_loglike_std(B, N, p_t.data_ptr(), o_t.data_ptr(), s_t.data_ptr(), chi2.data_ptr(), logL.data_ptr(), _stream(torch)))
        torch.cuda.synchronize()
        c, l = chi2.cpu().numpy(), logL.cpu().numpy()
        act = o > 0.0                                                # (False for NaN)
        r = np.where(act, (pred.astype(ld) - np.where(act, o, 1.0).astype(ld)) / sd.astype(ld), ld(0))
        c_ref = (r * r).sum(axis=1)
        lnsd = np.where(act, np.log(sd.astype(ld)), ld(0))
        na = act.sum(axis=1)
        l_ref = -0.5 * na * np.log(2 * ld(np.pi)) - lnsd.sum(axis=1) - 0.5 * c_ref
        u = ld(2.0) ** -52
        assert np.all(np.abs(c.astype(ld) - c_ref) <= (N + 8) * u * c_ref), (N, B, c, c_ref)
        l_mag = 0.5 * na * np.log(2 * ld(np.pi)) + np.abs(lnsd).sum(axis=1) + 0.5 * c_ref
        assert np.all(np.abs(l.astype(ld) - l_ref) <= (N + 16) * u * l_mag), (N, B, l, l_ref)
        none = na == 0
        assert np.all(c[none] == 0.0) and np.all(l[none] == 0.0)
    assert cases[1][B // 2].size == N and not (cases[1][B // 2] > 0.0).any()
