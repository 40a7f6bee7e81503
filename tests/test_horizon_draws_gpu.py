"""Joint draws of horizons on the device (csrc/gbp_horizon_draw.h k_horizon_filter / k_horizon_walk, gbp_horizon_draw) against the
numpy rule horizons.draw_reference: the walks with ``==`` wherever the rule's own margin says the device's exp cannot have tipped a
draw, the filter within the reference's own rounding, every instance of the filter, repeated and regrouped calls, the drivers and the
C entry's refusals."""
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, horizons as hz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SURVEY = os.path.join(GOLDEN, "device_survey_0.0.h5")
NS = (1, 2, 37)                                   # three sequences in one launch
PTR = np.concatenate([[0], np.cumsum(NS)])
NS_LARGEST = (1, 2, 9)                            # at S >= 513, where the numpy rule costs seconds per ten soundings
DZ, SLOPE, SWITCH = 0.5, 0.05, 2.3
EPS = 2.0 ** -52
MARGIN, CAP = 1e-9, 0.01                          # a (realisation, sequence) below MARGIN is left out; at most CAP of them may be


def _case(S, absent, seed, PTR=PTR, at=(5, 10, 20)):
    """The generator of tests/test_horizons_gpu.py: scores and steps of the three sequences, made once in numpy for both sides.  The
    long sequence has a repeated position (a zero distance, clamped), and two steps of the surface beyond the whole axis, one of each
    sign."""
    rng = np.random.default_rng(seed)
    total = int(PTR[-1])
    score = rng.normal(0.0, 2.0, (total, S))
    ab = rng.normal(0.0, 2.0, total) if absent else None
    x = np.cumsum(rng.uniform(5.0, 40.0, total))
    surface = np.cumsum(rng.normal(0.0, 1.0, total))
    r0 = int(PTR[2])
    i, j, k = (r0 + n for n in at)
    x[i + 1:] -= x[i + 1] - x[i]                                           # soundings at[0] and at[0] + 1 of the long sequence coincide
    surface[i + 1:] -= surface[i + 1] - surface[i]
    x[i + 1], surface[i + 1] = x[i], surface[i]                            # (exactly)
    surface[j + 1:] += S * DZ + 3.0                                        # |d| > S dz, upward
    surface[k + 1:] -= S * DZ + 3.25                                       # and downward
    g, d = hz.steps(x, np.zeros(total), surface, slope=SLOPE, ptr=PTR)
    assert g[i] == 1.0 / SLOPE and d[i] == 0.0 and d[j] > S * DZ and d[k] < -S * DZ
    return score, ab, g, d


def _device(ptr, score, ab, g, d, R, seed=7, row_key=None, dz=DZ, switch=SWITCH):
    dev = torch.device("cuda", 0)
    raw = hz.draw(np.asarray(ptr, dtype=np.int64), torch.as_tensor(score).to(dev), None if ab is None else torch.as_tensor(ab).to(dev), g, d, dz,
                  switch, R, seed=seed, row_key=row_key)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in raw.items()}


def _same_walks(got, ref, ptr):
    """draw_state == in every (realisation, sequence) whose margin >= MARGIN; returns how many were left out, and of how many."""
    out = 0
    for l, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        sure = ref["margin"][:, l] >= MARGIN
        out += int((~sure).sum())
        assert np.array_equal(got["draw_state"][sure, a:b], ref["draw_state"][sure, a:b]), "sequence %d" % l
    return out, ref["margin"].size


SHAPES = [(1, 5), (2, 65), (63, 300), (64, 64), (65, 63), (257, 129), (513, 65), (2048, 65)]


@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("S,R", SHAPES)
def test_draws_against_the_rule(S, R, absent):
    """Case seed 100 + S + absent, draw seed 7.  The walks with == where the margin allows (at most 1 % may be left out; the count is
    printed); ``filtered`` within max(16 e, 16 * 2^-52) of the long-double rule, e being the fp64 rule's own distance from it."""
    ns = NS_LARGEST if S >= 513 else NS
    ptr = np.concatenate([[0], np.cumsum(ns)])
    score, ab, g, d = _case(S, absent, 100 + S + absent, ptr, (1, 3, 6) if S >= 513 else (5, 10, 20))
    got = _device(ptr, score, ab, g, d, R)
    ref = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, R, seed=7)
    SA = S + absent
    assert got["draw_state"].shape == (R, int(ptr[-1])) and got["draw_state"].dtype == np.int32 and got["filtered"].shape == (int(ptr[-1]), SA)
    assert got["draw_state"].min() >= 0 and got["draw_state"].max() <= SA - 1
    left, of = _same_walks(got, ref, ptr)
    ld = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 1, seed=7, dtype=np.longdouble)
    e = float(np.abs(ref["filtered"] - ld["filtered"]).max())
    bound = max(16.0 * e, 16.0 * EPS)
    dist = float(np.abs(got["filtered"] - ld["filtered"]).max())
    print("S=%d R=%d absent=%d: %d of %d walks left out (smallest margin %.3g); filtered: e=%.3g bound=%.3g device distance=%.3g"
          % (S, R, absent, left, of, float(ref["margin"].min()), e, bound, dist))
    assert left <= CAP * of
    assert dist <= bound
    assert float(np.abs(got["scale"] / ld["scale"].astype(np.float64) - 1.0).max()) <= 64.0 * EPS


@pytest.mark.parametrize("S", [127, 128, 255, 256, 513, 769, 1025, 1281, 1537, 1793, 2047])
def test_every_instance_of_the_filter(S, absent=True):
    """One state count per instance of the filter, NJ = ceil((S + 1) / 256) = 1 .. 8 (the list of tests/test_horizon_graph_gpu.py's
    test_every_instance_of_the_sweep, and the last count of NJ = 8; NJ = 9 is S = 2048 above), with the absent state, on a path of three
    soundings."""
    rng = np.random.default_rng(S + absent)
    score = rng.normal(0.0, 2.0, (3, S))
    ab = rng.normal(0.0, 2.0, 3) if absent else None
    g, d = np.array([0.4, 1.1, 1.0]), np.array([3.2, -7.7, 0.0])
    R = 33
    got = _device([0, 3], score, ab, g, d, R, seed=S)
    ref = hz.draw_reference([0, 3], score, ab, g, d, DZ, SWITCH, R, seed=S)
    left, of = _same_walks(got, ref, np.array([0, 3]))
    print("S=%d absent=%d: %d of %d walks left out (smallest margin %.3g)" % (S, absent, left, of, float(ref["margin"].min())))
    assert left <= CAP * of
    ld = hz.draw_reference([0, 3], score, ab, g, d, DZ, SWITCH, 1, seed=S, dtype=np.longdouble)
    e = float(np.abs(ref["filtered"] - ld["filtered"]).max())                 # the bound of the main test: the rule's own rounding
    assert float(np.abs(got["filtered"] - ld["filtered"]).max()) <= max(16.0 * e, 16.0 * EPS)
    assert float(np.abs(got["scale"] / ld["scale"].astype(np.float64) - 1.0).max()) <= 64.0 * EPS


def test_a_call_repeats_its_bits_and_does_not_depend_on_its_shape():
    S = 65
    score, ab, g, d = _case(S, True, 42)
    seed, key = (0xDEADBEEF << 32) | 0x1234567, np.arange(int(PTR[-1]), dtype=np.int64) * (1 << 33) + 7      # non-zero high words
    a = _device(PTR, score, ab, g, d, 65, seed=seed, row_key=key)
    b = _device(PTR, score, ab, g, d, 65, seed=seed, row_key=key)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    one = _device(PTR, score, ab, g, d, 1, seed=seed, row_key=key)
    many = _device(PTR, score, ab, g, d, 300, seed=seed, row_key=key)                                       # two workgroups per sequence
    assert np.array_equal(one["draw_state"], a["draw_state"][:1]) and np.array_equal(many["draw_state"][:65], a["draw_state"])
    assert np.array_equal(one["filtered"], a["filtered"])
    ref = hz.draw_reference(PTR, score, ab, g, d, DZ, SWITCH, 300, seed=seed, row_key=key)
    left, of = _same_walks(many, ref, PTR)
    assert left <= CAP * of
    # the long sequence alone, with its keys: the same draws; an empty sequence writes nothing and disturbs nothing
    r0 = int(PTR[2])
    alone = _device([0, 0, 37], score[r0:], ab[r0:], g[r0:], d[r0:], 65, seed=seed, row_key=key[r0:])
    assert np.array_equal(alone["draw_state"], a["draw_state"][:, r0:]) and np.array_equal(alone["filtered"], a["filtered"][r0:])
    # the default key is the row index
    assert np.array_equal(_device(PTR, score, ab, g, d, 9)["draw_state"], _device(PTR, score, ab, g, d, 9, row_key=np.arange(int(PTR[-1])))["draw_state"])
    # no sequence at all: nothing is launched
    dev = torch.device("cuda", 0)
    none = hz.draw([0], torch.zeros((0, 3), dtype=torch.float64, device=dev), None, [], [], DZ, SWITCH, 2)
    assert none["draw_state"].shape == (2, 0) and none["filtered"].shape == (0, 3)


def _planted_lines(seed=0):
    """Three lines of 40 soundings over one planted horizon with an absent stretch, the evidence bimodal in places."""
    rng = np.random.default_rng(seed)
    L, n, S = 3, 40, 48
    N = L * n
    x = np.tile(25.0 * np.arange(n), L)
    y = np.repeat(100.0 * np.arange(L), n)
    surface = 5.0 * np.sin(x / 400.0) + rng.normal(0.0, 0.2, N)
    true = np.floor((surface + 12.0 + 3.0 * np.sin(x / 300.0)) / DZ).astype(np.int64)
    assert true.min() >= 0 and true.max() < S
    at = np.where(rng.uniform(size=N) < 0.3, rng.integers(0, S, N), true)
    evidence = 0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2)
    gone = (x > 300.0) & (x < 500.0)
    evidence[gone] = 0.01
    absent = np.where(gone, 3.0, 0.05)
    edges = np.arange(S + 9) * DZ                                            # the window below leaves cells out on either side
    full = np.zeros((N, S + 8))
    full[:, 4:4 + S] = evidence
    return x, y, surface, full, absent, edges, np.arange(L + 1) * n, (edges[4], edges[4 + S])


def test_track_with_draws():
    x, y, surface, evidence, absent, edges, ptr, between = _planted_lines()
    dev = torch.device("cuda", 0)
    ev, ab = torch.as_tensor(evidence).to(dev), torch.as_tensor(absent).to(dev)
    R, N, L = 200, evidence.shape[0], ptr.size - 1
    plain = hz.track(ev, x, y, surface, edges, absent=ab, between=between, switch=SWITCH, ptr=ptr)
    r = hz.track(ev, x, y, surface, edges, absent=ab, between=between, switch=SWITCH, ptr=ptr, draws=R, seed=3)
    assert set(r) - set(plain) == {"draw_cell", "draw_depth", "draw_elevation", "draw_log_score"}
    for k in plain:                                                          # draws changes no other output (NaN: absent, on both sides)
        assert torch.equal(torch.isnan(plain[k]), torch.isnan(r[k])) and torch.equal(torch.nan_to_num(plain[k]), torch.nan_to_num(r[k])), k
    cell = r["draw_cell"].cpu().numpy()
    assert cell.shape == (R, N) and cell.dtype == np.int32 and cell.min() == -1 and cell[cell >= 0].min() >= 4 and cell.max() < 52
    depth, elev = r["draw_depth"].cpu().numpy(), r["draw_elevation"].cpu().numpy()
    assert np.array_equal(np.isnan(depth), cell < 0) and np.array_equal(depth[cell >= 0], (cell[cell >= 0] + 0.5) * DZ)
    assert np.array_equal(elev[cell >= 0], np.broadcast_to(surface, (R, N))[cell >= 0] - depth[cell >= 0])
    # against the rule on the device's own scores
    lo, hi = hz.window(edges, between)
    score, a_s = (v.cpu().numpy() for v in hz.evidence_scores(ev[:, lo:hi], ab))
    g, d = hz.steps(x, y, surface, ptr=ptr)
    ref = hz.draw_reference(ptr, score, a_s, g, d, DZ, SWITCH, R, seed=3)
    state = np.where(cell < 0, hi - lo, cell - lo)
    left, of = _same_walks(dict(draw_state=state), ref, ptr)
    assert left <= CAP * of
    # draw_log_score: no path scores more than the most probable one; N * 2^-52 * sum |terms| covers the order of the sums
    ls, top = r["draw_log_score"].cpu().numpy(), r["log_score"].cpu().numpy()
    assert ls.shape == (R, L)
    terms = np.abs(np.concatenate([score, a_s[:, None]], axis=1)).max(axis=1)
    for l in range(L):
        n = int(ptr[l + 1] - ptr[l])
        slack = n * EPS * (terms[ptr[l]:ptr[l + 1]].sum() + n * max(SWITCH, float(np.abs(ls[:, l]).max())))
        assert np.all(ls[:, l] <= top[l] + slack)
    host = hz.draw_log_scores(torch.as_tensor(state), ptr, torch.as_tensor(score), torch.as_tensor(a_s), g, d, DZ, SWITCH).numpy()
    assert np.allclose(ls, host, rtol=0, atol=1e-10)
    p = np.exp(ls - r["log_partition"].cpu().numpy()[None, :])
    assert np.all(p > 0.0) and np.all(p < 1.0)
    # the share of the draws per sounding against the smoothed marginals: 5 sigma of R draws (+ the rounding of the marginals)
    share_absent = (cell < 0).mean(axis=0)
    m = r["absent_probability"].cpu().numpy()
    assert np.all(np.abs(share_absent - m) <= 5.0 * np.sqrt(np.maximum(m * (1.0 - m), 1.0 / R) / R) + 1e-9)
    # what the draws are for
    s = hz.draw_summary(r["draw_cell"], edges, x, y, ptr)
    want = hz.draw_summary_reference(cell, edges, x, y, ptr)
    for k in want:
        assert s[k].device.type == "cuda" and np.allclose(s[k].cpu().numpy(), want[k], rtol=1e-12, atol=1e-9), k
    assert float(s["longest_gap"].median()) >= 100.0 and hz.connected(r["draw_cell"], 0, 5) > hz.connected(r["draw_cell"], 10, 22)


def test_from_products_and_the_command_line(tmp_path):
    from geobipy_amd import hdf, line_products as lp
    arrays, _ = hdf.load_results(SURVEY)
    if lp._key(arrays, lp.INTERFACES + "/values/data") is None:
        pytest.skip("the golden container holds no interface histogram")
    wins = [(5.0, 60.0), (60.0, 115.0), (20.0, 100.0)]                       # two windows of 110 cells, one of 160
    plain = hz.from_products(SURVEY, wins, absent=True)
    r = hz.from_products(SURVEY, wins, absent=True, draws=4, seed=3)
    N = 8
    assert r["draw_cell"].shape == (3, 4, N) and r["draw_depth"].shape == (3, 4, N) and r["draw_log_score"].shape == (3, 4)
    for k in plain:
        a, b = plain[k], r[k]
        assert (torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) if torch.is_tensor(a) else np.array_equal(a, b)), k
    depth = r["draw_depth"].cpu().numpy()
    for h, (d0, d1) in enumerate(wins):
        here = ~np.isnan(depth[h])
        assert np.all((depth[h][here] >= d0) & (depth[h][here] < d1))
        one = hz.from_products(SURVEY, [wins[h]], absent=True, draws=4, seed=3)
        if h == 0:                                                           # the key of window 0 is the sounding index, alone or not
            assert torch.equal(one["draw_cell"][0], r["draw_cell"][h])
    # windows 0 and 1 have the same state count and share a launch; their keys differ by N: the rule with those keys
    prob, edges, x, y, s = hz._read(SURVEY, None)
    e = torch.as_tensor(np.nan_to_num(prob)).to(torch.device("cuda", 0))
    g, d = hz.steps(x, y, s)
    for h in (0, 1):
        lo, hi = hz.window(edges, wins[h])
        score, a_s = (v.cpu().numpy() for v in hz.evidence_scores(e[:, lo:hi], (e.sum(1) - e[:, lo:hi].sum(1)).clamp(min=0.0)))
        ref = hz.draw_reference([0, N], score, a_s, g, d, 0.5, 4.6, 4, seed=3, row_key=np.arange(N) + h * N)
        cell = r["draw_cell"][h].cpu().numpy()
        sure = ref["margin"][:, 0] >= MARGIN
        assert sure.all() and np.array_equal(np.where(cell < 0, hi - lo, cell - lo), ref["draw_state"])
    # the command line on a copy
    copy = str(tmp_path / "0.0.h5")
    shutil.copy(SURVEY, copy)
    written = hz.main([str(tmp_path), "--between", "5", "60", "--between", "60", "115", "--absent", "--draws", "4", "--seed", "3"])
    assert written == [str(tmp_path / "0.0.horizons.npz")] and os.path.exists(written[0])
    f = hz.load(written[0])
    assert np.array_equal(f["draw_cell"], r["draw_cell"][:2].cpu().numpy()) and np.array_equal(f["draw_log_score"], r["draw_log_score"][:2].cpu().numpy())
    assert np.array_equal(np.nan_to_num(f["draw_depth"]), np.nan_to_num(depth[:2])) and np.array_equal(f["cell"], plain["cell"][:2].cpu().numpy())


def test_c_entry_refusals_leave_the_outputs_alone():
    S, R = 5, 3
    score, ab, g, d = _case(S, True, 1)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(dev)      # noqa: E731
    total = int(PTR[-1])
    a = dict(ptr=t(PTR, torch.int64), score=t(score), ab=t(ab), g=t(g), d=t(d), filtered=torch.full((total, S + 1), 7.0, dtype=torch.float64, device=dev),
             scale=torch.full((total,), 7.0, dtype=torch.float64, device=dev), state=torch.full((R, total), 7, dtype=torch.int32, device=dev))
    st = torch.cuda.current_stream().cuda_stream
    err = lib.gbp_last_error

    def call(L=3, ptr=a["ptr"], total_n=total, max_n=37, S=S, dz=DZ, score=a["score"], switch=SWITCH, n_draws=R, filtered=a["filtered"], state=a["state"]):
        p = lambda v: None if v is None else v.data_ptr()                     # noqa: E731
        return lib.gbp_horizon_draw(L, p(ptr), total_n, max_n, S, dz, p(score), a["ab"].data_ptr(), a["g"].data_ptr(), a["d"].data_ptr(), switch, None, 0,
                                    n_draws, p(filtered), a["scale"].data_ptr(), p(state), st)

    for kw, word in ((dict(L=-1), b"L must"), (dict(S=0), b"S must"), (dict(S=2049), b"S must"), (dict(n_draws=0), b"n_draws must"),
                     (dict(n_draws=65537), b"n_draws must"), (dict(dz=0.0), b"dz"), (dict(switch=-1.0), b"switch"), (dict(max_n=41), b"total_n"),
                     (dict(total_n=3 * 37 + 1), b"total_n"), (dict(ptr=None), b"ptr is NULL"), (dict(score=None), b"NULL pointer (score"),
                     (dict(filtered=None), b"NULL pointer (filtered"), (dict(state=None), b"draw_state is NULL")):
        assert call(**kw) == -1 and b"gbp_horizon_draw" in err() and word in err(), kw
    assert call(L=0) == 0
    torch.cuda.synchronize()
    assert bool((a["filtered"] == 7.0).all()) and bool((a["scale"] == 7.0).all()) and bool((a["state"] == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    ref = hz.draw_reference(PTR, score, ab, g, d, DZ, SWITCH, R, seed=0)
    assert ref["margin"].min() >= MARGIN and np.array_equal(a["state"].cpu().numpy(), ref["draw_state"])
    assert bool((a["scale"] != 7.0).all())


# ---- across lines: gbp_horizon_graph_draw against horizons.graph_draw_reference --------------------------------------------------------

from geobipy_amd import sections  # noqa: E402
from test_horizon_draws import check_lattice, lattice_case  # noqa: E402
from test_horizon_graph import horizon_inputs, planted_horizon, PER_LINE  # noqa: E402
from test_spatial_sections import lattice_graph, line_graph, star_graph  # noqa: E402

GRAPH_SWITCH = 1.5
GRAPHS = {
    "line": lambda: (line_graph()[0], line_graph()[1], 6, [0, 6]),
    "cut_line": lambda: (line_graph()[0], line_graph()[1], 6, [0, 1, 3, 6]),                  # sequences of 1, 2, 3: two steps become cross edges
    "star_singletons": lambda: (star_graph()[0], star_graph()[1], 5, [0, 1, 2, 3, 4, 5]),
    "lattice": lambda: (lattice_graph()[0], lattice_graph()[1], 12, [0, 4, 8, 12]),
    "isolated_and_empty": lambda: (np.array([1, 1, 2, 3, 4]), np.array([2, 5, 3, 4, 5]), 7, [0, 1, 4, 4, 6, 7]),
    "three_adjacent": lambda: (np.array([0, 0, 0, 1, 2, 2, 4]), np.array([1, 2, 4, 3, 3, 4, 5]), 6, [0, 2, 4, 6]),
}
GRAPH_RS, GRAPH_SWEEPS = (5, 64, 65, 130), (0, 1, 3)


def _graph_device(eu, ev, g, d, dz, score, ab, ptr, R, **kw):
    dev = torch.device("cuda", 0)
    out = hz.graph_draw(eu, ev, g, d, dz, GRAPH_SWITCH, torch.as_tensor(score).to(dev), None if ab is None else torch.as_tensor(ab).to(dev),
                        np.asarray(ptr, dtype=np.int64), R, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _graph_case(name, S, absent):
    eu, ev, N, ptr = GRAPHS[name]()
    rng = np.random.default_rng(1000 + 7 * S + absent + 100 * sorted(GRAPHS).index(name))
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, absent)
    return eu, ev, g, d, dz, score, ab, np.asarray(ptr, dtype=np.int64), N


def _graph_against_the_rule(name, S, absent, Rs, sweeps):
    eu, ev, g, d, dz, score, ab, ptr, N = _graph_case(name, S, absent)
    left = of = 0
    for T in sweeps:
        ref = hz.graph_draw_reference(eu, ev, g, d, dz, GRAPH_SWITCH, score, ab, ptr, max(Rs), seed=7, sweeps=T)     # (a draw does not depend on R)
        for R in Rs:
            got = _graph_device(eu, ev, g, d, dz, score, ab, ptr, R, seed=7, sweeps=T, filtered=True)
            assert got["draw_state"].shape == (R, N) and got["draw_state"].dtype == np.int32 and got["filtered"].shape == (R, N, S + absent)
            assert got["draw_state"].min() >= 0 and got["draw_state"].max() <= S + absent - 1
            sure = ref["margin"][:R].min(axis=1) >= MARGIN                    # a whole realisation is left out when any of its margins is small
            left, of = left + int((~sure).sum()), of + R
            assert np.array_equal(got["draw_state"][sure], ref["draw_state"][:R][sure]), (name, S, absent, R, T)
            assert np.allclose(got["filtered"][sure], ref["filtered"][:R][sure], rtol=0, atol=1e-12), (name, S, absent, R, T)
    print("%s S=%d absent=%d: %d of %d realisations left out" % (name, S, absent, left, of))
    assert left <= CAP * of


@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("S", [1, 3, 63, 64, 65])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_draws_against_the_rule(name, S, absent):
    """S x absent x R in (5, 64, 65, 130) x sweeps in (0, 1, 3) on every graph: draw seed 7; a whole realisation is left out when any
    of its margins is < 1e-9, at most 1 % of them."""
    _graph_against_the_rule(name, S, absent, GRAPH_RS, GRAPH_SWEEPS)


@pytest.mark.parametrize("name", ["lattice", "three_adjacent"])
def test_graph_draws_with_two_owned_states(name):
    """S = 257 with R = 5: the second instance of the filter, conditioned."""
    _graph_against_the_rule(name, 257, True, (5,), (0, 1, 3))


def test_graph_blocks_continuation_and_trace_repeat_one_call():
    eu, ev, g, d, dz, score, ab, ptr, N = _graph_case("lattice", 9, True)
    key = np.arange(N, dtype=np.int64) + (5 << 32)
    kw = dict(seed=(3 << 40) + 1, row_key=key, filtered=True)
    one = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, **kw)
    again = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, **kw)
    two = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, block=40, **kw)
    tiny = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, budget_bytes=N * 10 * 8 * 3, **kw)      # blocks of 3
    for other in (again, two, tiny):
        assert np.array_equal(other["draw_state"], one["draw_state"]) and np.array_equal(other["filtered"], one["filtered"])
    half = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=2, **kw)
    rest = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, state=half["draw_state"], first_sweep=3, **kw)
    assert np.array_equal(rest["draw_state"], one["draw_state"]) and np.array_equal(rest["filtered"], one["filtered"])
    traced = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=4, trace=True, block=33, **kw)
    assert np.array_equal(traced["draw_state"], one["draw_state"]) and np.array_equal(traced["filtered"], one["filtered"])
    assert traced["log_score_trace"].shape == (5, 70) and traced["change_share"].shape == (4,) and np.all(traced["change_share"] > 0.0)
    assert np.array_equal(traced["log_score_trace"][-1], hz.graph_log_score(one["draw_state"], eu, ev, g, d, dz, GRAPH_SWITCH, score, ab))
    start = _graph_device(eu, ev, g, d, dz, score, ab, ptr, 70, sweeps=0, block=33, **kw)
    assert np.array_equal(traced["log_score_trace"][0], hz.graph_log_score(start["draw_state"], eu, ev, g, d, dz, GRAPH_SWITCH, score, ab))
    assert np.array_equal(start["filtered"][0], start["filtered"][69])        # the start's one alpha serves every realisation
    assert np.array_equal(_graph_device(eu, ev, g, d, dz, score, ab, ptr, 1, sweeps=4, **kw)["draw_state"], one["draw_state"][:1])
    none = hz.graph_draw(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), dz, GRAPH_SWITCH,
                         torch.zeros((0, 3), dtype=torch.float64, device=torch.device("cuda", 0)), None, [0], 2)
    assert none["draw_state"].shape == (2, 0)


def test_the_lattice_statistics_of_the_device_draws():
    eu, ev, g, d, dz, switch, score, ab, ptr = lattice_case()
    dev = torch.device("cuda", 0)
    for T in (6, 12):
        out = hz.graph_draw(eu, ev, g, d, dz, switch, torch.as_tensor(score).to(dev), torch.as_tensor(ab).to(dev), ptr, 4096, seed=4, sweeps=T)
        z, zp = check_lattice(out["draw_state"].cpu().numpy(), "lattice on the device, %d sweeps" % T)
        assert z <= 5.0 and zp <= 5.0


def test_spatial_with_draws_on_the_planted_lines():
    evidence, x, y, surface, edges, ptr, cell = planted_horizon()
    dev = torch.device("cuda", 0)
    ev_d = torch.as_tensor(evidence).to(dev)
    R, N, T = 64, evidence.shape[0], 8
    plain = hz.spatial(ev_d, x, y, surface, edges, max_distance=150.0, ptr=ptr, sweeps=16)
    r = hz.spatial(ev_d, x, y, surface, edges, max_distance=150.0, ptr=ptr, sweeps=16, draws=R, seed=1)
    assert set(r) - set(plain) == {"draw_cell", "draw_depth", "draw_elevation", "draw_log_score", "draw_share", "draw_change_share"}
    for k in plain:                                                          # draws changes no other output
        a, b = plain[k], r[k]
        assert (torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) if torch.is_tensor(a) else np.array_equal(a, b)), k
    dc = r["draw_cell"].cpu().numpy()
    assert dc.shape == (R, N) and dc.dtype == np.int32 and r["draw_depth"].shape == (R, N) and r["draw_log_score"].shape == (R,)
    assert r["draw_change_share"].shape == (T,) and r["draw_share"].shape == (N, evidence.shape[1])
    share = np.stack([np.bincount(dc[:, s], minlength=evidence.shape[1]) for s in range(N)]) / R      # recounted on the host (no absent state here)
    assert np.array_equal(r["draw_share"].cpu().numpy(), share)
    middle = np.arange(PER_LINE, 2 * PER_LINE)
    on_graph = float((dc[:, middle] == cell[middle][None, :]).mean())
    line = hz.track(ev_d, x, y, surface, edges, ptr=ptr, draws=R, seed=1)["draw_cell"].cpu().numpy()
    on_alone = float((line[:, middle] == cell[middle][None, :]).mean())
    print("planted cell of the middle line: %.3f of the line-alone draws, %.3f of the graph draws" % (on_alone, on_graph))
    assert on_alone < on_graph and on_graph > 0.5
    # draw_log_score <= log_score (the most probable surface found) within N * 2^-52 * sum |terms|
    ls, top = r["draw_log_score"].cpu().numpy(), float(r["log_score"])
    score = hz.evidence_scores(ev_d)[0].cpu().numpy()
    assert np.all(ls <= top + N * EPS * (np.abs(score).max(axis=1).sum() + 57 * 4.6 + np.abs(ls).max()))
    # against the rule on the device's own scores
    eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=150.0)
    g, d, _ = hz.graph_steps(x, y, surface, eu, ev)
    ref = hz.graph_draw_reference(eu, ev, g, d, 1.0, 4.6, score, None, ptr, R, seed=1, sweeps=T)
    sure = ref["margin"].min(axis=1) >= MARGIN
    assert (~sure).sum() <= CAP * R and np.array_equal(dc[sure], ref["draw_state"][sure])
    assert np.array_equal(ls[sure], hz.graph_log_score(ref["draw_state"][sure], eu, ev, g, d, 1.0, 4.6, score))


def test_the_command_line_draws_on_the_graph(tmp_path):
    for name in ("0.0.h5", "1.0.h5"):                                          # two lines (at the same places: the cross edges are clamped)
        shutil.copy(SURVEY, str(tmp_path / name))
    wins = [(5.0, 60.0), (60.0, 115.0)]
    written = hz.main([str(tmp_path), "--between", "5", "60", "--between", "60", "115", "--absent", "--spatial", "10", "--sweeps", "4", "--draws", "4",
                       "--seed", "3", "--draw-sweeps", "2"])
    assert written == [str(tmp_path / "survey.horizons.npz")] and os.path.exists(written[0])
    f = hz.load(written[0])
    N = 16
    assert f["draw_cell"].shape == (2, 4, N) and f["draw_depth"].shape == (2, 4, N) and f["draw_log_score"].shape == (2, 4)
    assert f["draw_change_share"].shape == (2, 2) and f["draw_share_0"].shape == (N, 111) and f["draw_share_1"].shape == (N, 111)
    for h, (d0, d1) in enumerate(wins):
        here = ~np.isnan(f["draw_depth"][h])
        assert np.array_equal(here, f["draw_cell"][h] >= 0) and np.all((f["draw_depth"][h][here] >= d0) & (f["draw_depth"][h][here] < d1))
        assert np.array_equal(f["draw_share_%d" % h].sum(axis=1), np.ones(N))
    paths = [str(tmp_path / "0.0.h5"), str(tmp_path / "1.0.h5")]
    direct = hz.spatial_from_products(paths, wins, 10.0, sweeps=4, absent=True, draws=4, seed=3, draw_sweeps=2)
    assert set(direct) == set(f) and all(np.array_equal(_args_host(direct[k]), f[k], equal_nan=True) for k in f)
    plain = hz.spatial_from_products(paths, wins, 10.0, sweeps=4, absent=True)
    assert set(f) - set(plain) == {"draw_cell", "draw_depth", "draw_elevation", "draw_log_score", "draw_change_share", "draw_share_0", "draw_share_1"}
    assert all(np.array_equal(_args_host(plain[k]), f[k], equal_nan=True) for k in plain)      # draws changes no other output
    # the key of window h is sounding + h * N: the second window alone is window 0 of its own list, and draws with other keys
    second = hz.spatial_from_products(paths, wins[1:], 10.0, sweeps=4, absent=True, draws=4, seed=3, draw_sweeps=2)
    assert np.array_equal(second["cell"].cpu().numpy()[0], f["cell"][1]) and second["draw_cell"].shape == (1, 4, N)


def _args_host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def test_graph_entry_refusals_leave_the_outputs_alone():
    eu, ev, g, d, dz, score, ab, ptr, N = _graph_case("lattice", 3, True)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R, SA, E = 3, 4, eu.size
    _, step_edge, cross = sections.check_lines(eu, ev, ptr, N, "test")
    cross_ptr, cross_edge = sections.cross_incoming(eu, ev, cross, N)
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(dev)      # noqa: E731
    i = {k: t(v, torch.int32) for k, v in dict(eu=eu, ev=ev, step=step_edge, cptr=cross_ptr, cedge=cross_edge,
                                               colptr=np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n_colours))]),
                                               colline=np.argsort(colour, kind="stable")).items()}
    theta, tg, td, tptr = t(np.concatenate([score, ab[:, None]], axis=1), torch.float64), t(g, torch.float64), t(d, torch.float64), t(ptr, torch.int64)
    alpha, scale = torch.full((R, N, SA), 7.0, dtype=torch.float64, device=dev), torch.full((R, N), 7.0, dtype=torch.float64, device=dev)
    state = torch.full((R, N), 7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    err = lib.gbp_last_error

    def call(N=N, S=3, L=3, n_colours=n_colours, n_draws=R, first_draw=0, first_sweep=0, sweeps=2, theta=theta, alpha=alpha, colline=i["colline"], dz=dz):
        p = lambda v: None if v is None else v.data_ptr()                     # noqa: E731
        return lib.gbp_horizon_graph_draw(N, E, S, 1, dz, GRAPH_SWITCH, p(i["eu"]), p(i["ev"]), p(theta), p(tg), p(td), L, p(tptr), p(i["step"]),
                                          p(i["cptr"]), p(i["cedge"]), n_colours, p(i["colptr"]), p(colline), None, 7, n_draws, first_draw, first_sweep,
                                          sweeps, p(alpha), p(scale), p(state), st)

    for kw, word in ((dict(N=-1), b"N must"), (dict(S=0), b"S must"), (dict(S=2049), b"S must"), (dict(dz=0.0), b"dz"), (dict(L=0), b"L >= 1"),
                     (dict(n_draws=0), b"n_draws must"), (dict(n_draws=65537), b"n_draws must"), (dict(first_draw=65535), b"first_draw"),
                     (dict(first_sweep=3), b"sweeps"), (dict(sweeps=65536), b"sweeps"), (dict(n_colours=0), b"colour lists must cover"),
                     (dict(n_colours=4), b"colour lists must cover"), (dict(theta=None), b"NULL pointer (score"), (dict(alpha=None), b"NULL pointer (alpha"),
                     (dict(colline=None), b"NULL pointer (score")):
        assert call(**kw) == -1 and b"gbp_horizon_graph_draw" in err() and word in err(), kw
    torch.cuda.synchronize()
    assert bool((alpha == 7.0).all()) and bool((scale == 7.0).all()) and bool((state == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    ref = hz.graph_draw_reference(eu, ev, g, d, dz, GRAPH_SWITCH, score, ab, ptr, R, seed=7, sweeps=2)
    assert ref["margin"].min() >= MARGIN and np.array_equal(state.cpu().numpy(), ref["draw_state"])
    assert bool((alpha != 7.0).all()) and np.allclose(alpha.cpu().numpy(), ref["filtered"], rtol=0, atol=1e-12)
