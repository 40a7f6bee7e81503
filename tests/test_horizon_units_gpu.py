"""Horizon pairs on the device (csrc/gbp_horizon_unit.h k_unit_viterbi / k_unit_marginals, gbp_horizon_unit_track)
against the numpy rule horizons.unit_reference: the two picks and their score with ``==``, the marginals within the rule's own
rounding (its fp64 evaluation against its long-double evaluation), the degenerate launches, the public entry and the command line."""
import functools
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, horizons as hz
from test_horizons_gpu import DZ, EPS, SURVEY, SWITCH, _case

NS = (1, 2, 9)                                    # three sequences in one launch
PTR = np.concatenate([[0], np.cumsum(NS)])
SMAX = hz.MAX_UNIT_STATES
KEYS = ("marginal_top", "marginal_base", "marginal_thickness", "marginal_absent")


@functools.lru_cache(maxsize=None)
def _inputs(S, absent, thick):
    """Scores and steps, made once in numpy for both sides: the top's scores and the steps of tests/test_horizons_gpu.py::_case (a
    clamped zero distance, and surface steps beyond the whole axis in both directions), the base's and the thickness's beside them."""
    st, ab, g, d = _case(S, absent, 300 + S + absent, PTR, (1, 3, 6))
    rng = np.random.default_rng(900 + S)
    sb = rng.normal(0.0, 2.0, st.shape)
    ts = rng.normal(0.0, 1.0, S) if thick else None
    return st, sb, ts, ab, g, d


@functools.lru_cache(maxsize=None)
def _rule(S, mc, absent, thick, dtype):
    st, sb, ts, ab, g, d = _inputs(S, absent, thick)
    return hz.unit_reference(PTR, st, sb, g, d, DZ, SWITCH, min_cells=mc, thickness_score=ts, absent_score=ab, dtype=dtype)


def _device(st, sb, ts, ab, g, d, mc, dz=DZ, switch=SWITCH, marginals=True, ptr=PTR, **kw):
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64).to(dev)     # noqa: E731
    raw = hz._unit_launch(t(st), t(sb), t(ts), t(ab), np.asarray(ptr, dtype=np.int64), g, d, dz, switch, mc, marginals, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in raw.items()}


def _shapes():
    out = []
    for S in (1, 2, 3, 31, 64, 65, SMAX):
        for mc in sorted({0, min(1, S - 1), S - 1}):
            out.append((S, mc))
    return out


@pytest.mark.parametrize("thick", [False, True])
@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("S,mc", _shapes())
def test_kernels_against_the_rule(S, mc, absent, thick):
    """cell_top, cell_base and log_score with ==.  Every marginal within max(16 e, 16 * 2^-52) of the long-double rule, e = max |fp64
    rule - long-double rule| over the four marginals (the rule's own rounding), plus the a-priori term S * 2^-52 * value: the device
    sums the three projections of gamma -- and, like gbp_horizon_track, the normalising sums and the absent state's sums over the
    pairs -- by lanes and waves, in another order than numpy, and a sum of at most S^2 non-negative terms in any order is within
    about S * 2^-52 of itself per reduction level.  Each sounding's total mass is 1 within the same bound (with
    value = 1)."""
    st, sb, ts, ab, g, d = _inputs(S, absent, thick)
    got = _device(st, sb, ts, ab, g, d, mc)
    ref, ld = _rule(S, mc, absent, thick, np.float64), _rule(S, mc, absent, thick, np.longdouble)
    assert got["cell_top"].dtype == np.int32 and got["cell_base"].dtype == np.int32
    assert np.array_equal(got["cell_top"], ref["cell_top"]) and np.array_equal(got["cell_base"], ref["cell_base"])
    assert np.array_equal(got["log_score"], ref["log_score"])
    assert np.array_equal(ld["cell_top"], ref["cell_top"]) and np.array_equal(ld["cell_base"], ref["cell_base"])
    here = got["cell_top"] < S
    assert np.all((got["cell_base"] - got["cell_top"])[here] >= mc) and np.all(got["cell_base"][~here] == S) and (absent or here.all())
    e = max(float(np.abs(ref[k] - ld[k]).max()) for k in KEYS)
    bound = max(16.0 * e, 16.0 * EPS)
    for k in KEYS:
        want = ld[k].astype(np.float64)
        assert np.all(np.isfinite(want)) and got[k].shape == want.shape
        over = np.abs(got[k] - ld[k]).astype(np.float64) - (bound + S * EPS * want)
        print("S=%d mc=%d absent=%d thick=%d %s: e=%.3g bound=%.3g device distance=%.3g" % (S, mc, absent, thick, k, e, bound,
                                                                                          float(np.abs(got[k] - want).max())))
        assert float(over.max()) <= 0.0, k
    mass = got["marginal_top"].sum(axis=1) + got["marginal_absent"]
    assert float(np.abs(mass - 1.0).max()) <= bound + S * EPS
    assert np.all(got["marginal_thickness"][:, :mc] == 0.0)                  # no mass below min_cells
    if not absent:
        assert np.all(got["marginal_absent"] == 0.0)
    # log_partition: a sum of N logarithms, each good to a few ulp of itself and of its argument's relative error
    lp_bound = np.array([16.0 * EPS * (n + np.abs(np.log(ld["scale"][a:a + n].astype(np.float64))).sum()) for a, n in zip(PTR[:-1], NS)])
    lp_dist = np.abs(got["log_partition"] - ld["log_partition"]).astype(np.float64)
    print("log_partition distance=%.3g (bound %.3g)" % (lp_dist.max(), lp_bound.min()))
    assert np.all(lp_dist <= lp_bound)
    # scale: relative, against the rule's own rounding again -- behind a step of the surface beyond the whole axis s_n = exp(-T) of a
    # T of some hundreds, whose own rounding, a few 2^-52 T, is a relative error of s_n far above 2^-52 on both sides
    e_s = float(np.abs(ref["scale"] / ld["scale"] - 1.0).max())
    assert float(np.abs(got["scale"] / ld["scale"] - 1.0).max()) <= max(16.0 * e_s, 64.0 * EPS)


@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("mc", [0, 1, 3])
def test_exact_ties_follow_the_tie_order(absent, mc):
    """Integer scores, g dz = 1 exactly and d a multiple of dz: many paths score the same, and the device picks the pair the rule
    picks -- in both passes, into and out of the absent state, and at the end of the path."""
    rng = np.random.default_rng(19 + mc)
    S, total = 70, int(PTR[-1])
    st, sb = rng.integers(0, 3, (total, S)).astype(np.float64), rng.integers(0, 3, (total, S)).astype(np.float64)
    ab = rng.integers(0, 4, total).astype(np.float64) if absent else None
    ts = rng.integers(0, 2, S).astype(np.float64)
    g, d = np.full(total, 2.0), rng.integers(-4, 5, total) * 0.5
    got = _device(st, sb, ts, ab, g, d, mc, dz=0.5, switch=2.0, marginals=False)
    ref = hz.unit_reference(PTR, st, sb, g, d, 0.5, 2.0, min_cells=mc, thickness_score=ts, absent_score=ab, marginals=False)
    for k in ("cell_top", "cell_base", "log_score"):
        assert np.array_equal(got[k], ref[k]), k
    zero = np.zeros((total, S))
    flat = _device(zero, zero, None, np.zeros(total) if absent else None, g, 0.0 * d, mc, dz=0.5, switch=0.0, marginals=False)
    assert not flat["cell_top"].any() and np.all(flat["cell_base"] == mc)   # all ties: the first valid pair, never absent


def test_without_marginals_and_degenerate_launches():
    S, mc = 65, 2
    st, sb, ts, ab, g, d = _inputs(S, True, True)
    got = _device(st, sb, ts, ab, g, d, mc, marginals=False)
    ref = hz.unit_reference(PTR, st, sb, g, d, DZ, SWITCH, min_cells=mc, thickness_score=ts, absent_score=ab, marginals=False)
    assert set(got) == {"cell_top", "cell_base", "log_score"}
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    # sequences of one sounding each
    one = np.arange(4)
    got = _device(st[:3], sb[:3], ts, ab[:3], g[:3], d[:3], mc, ptr=one)
    ref = hz.unit_reference(one, st[:3], sb[:3], g[:3], d[:3], DZ, SWITCH, min_cells=mc, thickness_score=ts, absent_score=ab[:3])
    for k in ("cell_top", "cell_base", "log_score"):
        assert np.array_equal(got[k], ref[k]), k
    for k in KEYS + ("log_partition",):
        assert np.allclose(got[k], ref[k], rtol=0, atol=1e-13), k
    # a call repeated: equal bits
    a, b = _device(st, sb, ts, ab, g, d, mc), _device(st, sb, ts, ab, g, d, mc)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # L == 0: nothing is launched, the outputs keep their values; and a refusal before any launch
    lib = _lib.load()
    cell = torch.full((5,), -7, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    none = [None] * 7
    rc = lib.gbp_horizon_unit_track(0, None, 0, 0, S, mc, DZ, None, None, None, None, None, None, SWITCH, None, None, cell.data_ptr(),
                                    cell.data_ptr(), None, *none, stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((cell == -7).all())
    assert lib.gbp_horizon_unit_track(0, None, 0, 0, SMAX + 1, 0, DZ, None, None, None, None, None, None, SWITCH, None, None, None, None, None,
                                      *none, stream) != 0
    assert "1 .. %d " % SMAX in lib.gbp_last_error().decode()                # the message names the constant that is built
    assert lib.gbp_horizon_unit_track(0, None, 0, 0, S, S, DZ, None, None, None, None, None, None, SWITCH, None, None, None, None, None, *none,
                                      stream) != 0


def test_unit_on_the_device_and_refusals():
    rng = np.random.default_rng(4)
    NS3 = (7, 1, 10)
    ptr = np.concatenate([[0], np.cumsum(NS3)])
    N, nz = int(ptr[-1]), 41
    edges = np.arange(nz + 1) * 0.5
    e_top, e_base = rng.uniform(0.0, 1.0, (N, nz)), rng.uniform(0.0, 1.0, (N, nz))
    e_top[3] = 0.0                                                           # an empty sounding
    x, surface = 20.0 * np.arange(N), np.cumsum(rng.normal(0.0, 0.3, N))
    a_top, a_base = rng.uniform(0.0, 3.0, N), rng.uniform(0.0, 3.0, N)
    a_top[11:15], a_base[11:15] = 400.0, 400.0                               # a stretch where the unit is absent
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a).to(dev)                                 # noqa: E731
    args = dict(between=(2.0, 19.4), top_between=(2.0, 9.0), base_between=(7.0, 19.0), min_thickness=2.5, coarsen=3,
                absent=(t(a_top), t(a_base)), ptr=ptr)
    r = hz.unit(t(e_top), t(e_base), x, np.zeros(N), surface, edges, **args)
    # the rule on the same evidence: the window holds the cells 4 .. 38 less the trailing partial group -> 11 groups of 3 from cell 4
    lo, hi = hz.window(edges, (2.0, 19.4))
    assert (lo, hi) == (4, 39)
    S, C, mc = 11, 3, 2                                                      # ceil(2.5 / 1.5) = 2 cells
    centre = 0.5 * (edges[1:] + edges[:-1])

    def coarse(e, d0, d1):
        e = np.where((centre >= d0) & (centre < d1), e, 0.0)[:, lo:lo + S * C]
        return t(e).reshape(N, S, C).sum(dim=2)

    (s_top, b_top), (s_base, b_base) = (hz.evidence_scores(coarse(e, *w), t(ab)) for e, w, ab in ((e_top, (2.0, 9.0), a_top), (e_base, (7.0, 19.0), a_base)))
    g, d = hz.steps(x, np.zeros(N), surface, ptr=ptr)
    ref = hz.unit_reference(ptr, s_top.cpu().numpy(), s_base.cpu().numpy(), g, d, 1.5, 4.6, min_cells=mc, absent_score=(b_top + b_base).cpu().numpy())
    assert int(r["min_cells"]) == mc and np.allclose(r["cell_depth_edges"], 2.0 + 1.5 * np.arange(S + 1))
    ct, cb = r["top_cell"].cpu().numpy(), r["base_cell"].cpu().numpy()
    gone = ref["cell_top"] == S
    assert gone[11:15].all() and not gone.all()
    assert r["top_cell"].device.type == "cuda" and r["top_cell"].dtype == torch.int32
    assert np.array_equal(ct, np.where(gone, -1, lo + C * ref["cell_top"] + 1)) and np.array_equal(cb, np.where(gone, -1, lo + C * ref["cell_base"] + 1))
    assert np.array_equal(r["log_score"].cpu().numpy(), ref["log_score"])
    td, bd, th = (r[k].cpu().numpy() for k in ("top_depth", "base_depth", "thickness"))
    assert np.array_equal(np.isnan(td), gone) and np.array_equal(np.isnan(bd), gone) and np.array_equal(np.isnan(th), gone)
    assert np.allclose(td[~gone], 2.0 + 1.5 * (ref["cell_top"][~gone] + 0.5), rtol=0, atol=1e-12)
    assert np.allclose(th[~gone], 1.5 * (ref["cell_base"] - ref["cell_top"])[~gone], rtol=0, atol=1e-12) and th[~gone].min() >= 2.5
    assert np.allclose(r["top_elevation"].cpu().numpy()[~gone], surface[~gone] - td[~gone], rtol=0, atol=1e-12)
    assert np.allclose(r["base_elevation"].cpu().numpy()[~gone], surface[~gone] - bd[~gone], rtol=0, atol=1e-12)
    for k, want in (("top_marginal", "marginal_top"), ("base_marginal", "marginal_base"), ("thickness_marginal", "marginal_thickness"),
                    ("absent_probability", "marginal_absent"), ("log_partition", "log_partition")):
        assert np.allclose(r[k].cpu().numpy(), ref[want], rtol=0, atol=1e-12), k
    assert "pinched_probability" not in r and float(r["absent_probability"][12]) > 0.9
    mk = ref["marginal_thickness"]
    assert np.allclose(r["thickness_mean"].cpu().numpy(), (mk * (1.5 * np.arange(S))).sum(1) / mk.sum(1), rtol=0, atol=1e-10)
    p5, p50, p95 = (r["thickness_percentile_%d" % p].cpu().numpy() for p in (5, 50, 95))
    assert np.all(p5 <= p50) and np.all(p50 <= p95) and p5.min() >= 3.0
    assert np.all(r["top_depth_percentile_50"].cpu().numpy() < 9.5) and np.all(r["base_depth_percentile_50"].cpu().numpy() > 6.5)
    iv = hz.unit_intervals(r)
    assert iv["kind"] == "horizons" and np.array_equal(np.isnan(iv["top"]), gone) and np.all((iv["bottom"] - iv["top"])[~gone] >= 2.5)
    # split by whole sequences under a tiny budget: the bits of the unsplit launch; one sequence beyond it: refused
    need = hz.unit_bytes(10, S)
    split = hz.unit(t(e_top), t(e_base), x, np.zeros(N), surface, edges, budget_bytes=need, **args)
    for k, v in r.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, split[k]) or bool((torch.isnan(v) == torch.isnan(split[k])).all() and torch.equal(v.nan_to_num(), split[k].nan_to_num())), k
    with pytest.raises(ValueError, match="budget_bytes"):
        hz.unit(t(e_top), t(e_base), x, np.zeros(N), surface, edges, budget_bytes=need - 1, **args)
    # one evidence for both, no absent state, a unit that may pinch out
    same = hz.unit(t(e_top), None, x, np.zeros(N), surface, edges, between=(2.0, 19.9), min_thickness=0.0, marginals=True, ptr=ptr)
    assert "pinched_probability" in same and int(same["min_cells"]) == 0 and int(same["top_cell"].min()) >= 4
    assert bool((same["base_cell"] >= same["top_cell"]).all()) and float(same["absent_probability"].abs().max()) == 0.0
    quick = hz.unit(t(e_top), None, x, np.zeros(N), surface, edges, between=(2.0, 19.9), marginals=False, ptr=ptr)
    assert "top_marginal" not in quick and bool((quick["base_cell"] > quick["top_cell"]).all())
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        hz.unit(torch.as_tensor(e_top), None, x, np.zeros(N), surface, edges, between=(2.0, 19.9), ptr=ptr)
    with pytest.raises(ValueError, match="at most %d" % SMAX):
        hz.unit(t(np.ones((N, 200))), None, x, np.zeros(N), surface, np.arange(201) * 0.5, ptr=ptr)
    poisoned = np.zeros(36)
    poisoned[5] = np.nan
    with pytest.raises(ValueError, match="thickness_score must be finite"):
        hz.unit(t(e_top), None, x, np.zeros(N), surface, edges, between=(2.0, 19.9), thickness_score=poisoned, ptr=ptr)
    with pytest.raises(ValueError, match="min_thickness"):
        hz.unit(t(e_top), None, x, np.zeros(N), surface, edges, between=(2.0, 19.9), min_thickness=100.0, ptr=ptr)


def test_the_command_line(tmp_path):
    copy = str(tmp_path / "0.0.h5")
    shutil.copy(SURVEY, copy)
    written = hz.main([str(tmp_path), "--between", "5", "60", "--unit", "--coarsen", "2", "--min-thickness", "3", "--top-between", "5", "40",
                       "--base-between", "20", "60", "--absent"])
    assert written == [str(tmp_path / "0.0.unit.npz")] and os.path.exists(written[0]) and not os.path.exists(str(tmp_path / "0.0.horizons.npz"))
    f = hz.load(written[0])
    N, S = 8, 55
    for k in ("top_cell", "base_cell", "top_depth", "base_depth", "top_elevation", "base_elevation", "thickness", "absent_probability",
              "thickness_mean", "thickness_percentile_50", "top_depth_percentile_5", "base_depth_percentile_95", "scale"):
        assert f[k].shape == (N,), k
    assert f["top_marginal"].shape == (N, S) and f["base_marginal"].shape == (N, S) and f["thickness_marginal"].shape == (N, S)
    assert f["log_score"].shape == (1,) and f["log_partition"].shape == (1,) and int(f["min_cells"]) == 3 and "pinched_probability" not in f
    here = f["top_cell"] >= 0
    assert np.all(f["thickness"][here] >= 3.0) and np.all(np.isnan(f["thickness"][~here]))
    direct = hz.unit_from_products(SURVEY, (5.0, 60.0), absent=True, coarsen=2, min_thickness=3.0, top_between=(5.0, 40.0), base_between=(20.0, 60.0))
    assert np.array_equal(direct["top_cell"].cpu().numpy(), f["top_cell"]) and np.array_equal(direct["log_score"].cpu().numpy(), f["log_score"])
    for bad in (["--unit", "--between", "5", "60", "--between", "60", "115"], ["--unit", "--between", "5", "60", "--spatial", "300"],
                ["--unit", "--between", "5", "60", "--draws", "4"], ["--between", "5", "60", "--coarsen", "2"],
                ["--unit", "--between", "5", "60", "--top-between", "9", "8"]):
        with pytest.raises(SystemExit):
            hz.parse_args([str(tmp_path)] + bad)
