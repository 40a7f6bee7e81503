"""Joint draws of horizons along lines, on the host: the numpy rule horizons.draw_reference against the enumeration of every path and
against the long-double marginals, its filter against the formulas written out, the independence of a draw from the launch (R, the
grouping of sequences, the keys), the summaries of draws, every refusal, the C entries' refusals, the header and the parser; and the
rule across lines, horizons.graph_draw_reference: its start against draw_reference, a lattice with loops and a star against
enumeration, continuation, the planted lines."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import build, horizons as hz, sections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DZ, SWITCH = 0.5, 1.2


def _chain(N, S, absent, seed):
    rng = np.random.default_rng(seed)
    score = rng.normal(0.0, 1.0, (N, S))
    ab = rng.normal(0.0, 1.0, N) if absent else None
    g = rng.uniform(0.5, 2.0, N)
    d = rng.normal(0.0, 0.6, N)
    return score, ab, g, d


def _path_probabilities(score, ab, g, d, dz, switch):
    """Every path of one sequence and its probability, in long double: exp(node terms - pair costs), normalised."""
    N, S = score.shape
    SA = S + (ab is not None)
    theta = (score if ab is None else np.concatenate([score, ab[:, None]], axis=1)).astype(np.longdouble)
    paths = list(itertools.product(range(SA), repeat=N))
    p = np.zeros(len(paths), dtype=np.longdouble)
    for q, x in enumerate(paths):
        v = sum(theta[n, x[n]] for n in range(N))
        for n in range(N - 1):
            a, b = x[n], x[n + 1]
            v -= np.longdouble(g[n]) * abs(np.longdouble(d[n]) - (b - a) * np.longdouble(dz)) if a < S and b < S else (0.0 if a >= S and b >= S else switch)
        p[q] = np.exp(v)
    return paths, (p / p.sum()).astype(np.float64)


@pytest.mark.parametrize("absent", [False, True])
def test_path_frequencies_against_the_enumeration(absent):
    """N = 4, S = 3: 81 (256 with the absent state) paths; 4096 draws with a fixed seed; the worst |z| over the paths with an expected
    count >= 5 stays within 5."""
    N, S, R = 4, 3, 4096
    score, ab, g, d = _chain(N, S, absent, 11 + absent)
    paths, p = _path_probabilities(score, ab, g, d, DZ, SWITCH)
    r = hz.draw_reference([0, N], score, ab, g, d, DZ, SWITCH, R, seed=5)
    assert r["draw_state"].shape == (R, N) and r["draw_state"].dtype == np.int32 and r["margin"].shape == (R, 1)
    index = {x: q for q, x in enumerate(paths)}
    count = np.bincount([index[tuple(int(v) for v in row)] for row in r["draw_state"]], minlength=len(paths))
    keep = R * p >= 5.0
    z = (count - R * p)[keep] / np.sqrt(R * p * (1.0 - p))[keep]
    print("absent=%d: %d of %d paths expected >= 5 times, worst |z| = %.2f" % (absent, keep.sum(), len(paths), np.abs(z).max()))
    assert keep.sum() >= 20 and np.abs(z).max() <= 5.0
    # the test can tell the joint from the product of the marginals: the product's expected counts lie far outside the same bound
    m = hz.track_reference([0, N], score, ab, g, d, DZ, SWITCH)["marginal"]
    prod = np.array([np.prod([m[n, x[n]] for n in range(N)]) for x in paths])
    assert np.abs((R * prod - R * p)[keep] / np.sqrt(R * p * (1.0 - p))[keep]).max() > 5.0


@pytest.mark.parametrize("absent", [False, True])
def test_sounding_frequencies_against_the_long_double_marginals(absent):
    ptr, S, R = np.array([0, 1, 3, 10]), 5, 4096
    score, ab, g, d = _chain(10, S, absent, 3)
    r = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, R, seed=1)
    m = hz.track_reference(ptr, score, ab, g, d, DZ, SWITCH, dtype=np.longdouble)["marginal"].astype(np.float64)
    SA = S + absent
    freq = np.stack([np.bincount(r["draw_state"][:, n], minlength=SA) for n in range(10)]) / R
    z = (freq - m) / np.sqrt(np.maximum(m * (1.0 - m), 1e-12) / R)
    assert np.abs(z[R * m >= 5.0]).max() <= 5.0
    assert r["draw_state"].max() <= SA - 1 and r["draw_state"].min() >= 0


@pytest.mark.parametrize("absent", [False, True])
def test_filtered_is_alpha_of_the_formulas(absent):
    """alpha and s recomputed with scalar loops in the order the rule names, ==; s is also track_reference's ``scale``, bit for bit."""
    ptr, S = np.array([0, 2, 6]), 4
    score, ab, g, d = _chain(6, S, absent, 8)
    r = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 3)
    SA, ks = S + absent, np.exp(-SWITCH)
    for a, b in zip(ptr[:-1], ptr[1:]):
        prev = None
        for n in range(a, b):
            w = np.exp(np.append(score[n], ab[n]) if absent else score[n])
            if prev is None:
                u = w
            else:
                u = np.zeros(SA)
                for cp in range(S):
                    acc = 0.0
                    for c in range(S):
                        acc = acc + prev[c] * np.exp(-(g[n - 1] * abs(d[n - 1] - (cp - c) * DZ)))
                    u[cp] = w[cp] * (acc + prev[S] * ks if absent else acc)
                if absent:
                    acc = 0.0
                    for c in range(S):
                        acc = acc + prev[c] * ks
                    u[S] = w[S] * (acc + prev[S])
            s = u.sum()
            prev = u / s
            assert np.array_equal(r["filtered"][n], prev) and r["scale"][n] == s
    assert np.array_equal(r["scale"], hz.track_reference(ptr, score, ab, g, d, DZ, SWITCH)["scale"])


def test_a_draw_does_not_depend_on_the_launch():
    ptr, S = np.array([0, 5, 9]), 6
    score, ab, g, d = _chain(9, S, True, 21)
    seed, key = (0xDEADBEEF << 32) | 0x1234567, np.arange(9, dtype=np.int64) * (1 << 33) + 7        # non-zero high words
    big = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 70, seed=seed, row_key=key)
    small = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 9, seed=seed, row_key=key)
    assert np.array_equal(big["draw_state"][:9], small["draw_state"]) and np.array_equal(big["margin"][:9], small["margin"])
    # the second piece of the cut sequence, alone, with the same keys
    alone = hz.draw_reference([0, 4], score[5:], ab[5:], g[5:], d[5:], DZ, SWITCH, 70, seed=seed, row_key=key[5:])
    assert np.array_equal(alone["draw_state"], big["draw_state"][:, 5:]) and np.array_equal(alone["filtered"], big["filtered"][5:])
    assert np.array_equal(alone["margin"][:, 0], big["margin"][:, 1])
    # the default key is the row index; another seed or other keys give other draws
    assert np.array_equal(hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 70, seed=seed)["draw_state"],
                          hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 70, seed=seed, row_key=np.arange(9))["draw_state"])
    assert not np.array_equal(hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 70, seed=seed + (1 << 40), row_key=key)["draw_state"], big["draw_state"])
    assert not np.array_equal(hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 70, seed=seed, row_key=key + (1 << 32))["draw_state"], big["draw_state"])
    # the uniform is the section draws', counter (rho, key low, key high, 0): the last sounding's pick follows from it and alpha
    u = sections.philox_uniform(seed, np.arange(70), key[8])
    c = np.cumsum(big["filtered"][8])
    assert np.array_equal(big["draw_state"][:, 8], np.minimum((c[None, :] <= (u * c[-1])[:, None]).sum(axis=1), S))


def test_two_horizons_of_one_sounding_never_share_a_uniform():
    """The row-key convention: sounding index + horizon index * N.  Two horizons with the same evidence then draw differently, and a
    horizon keeps its draws whichever horizons share its launch."""
    N, S, H, R = 6, 5, 3, 40
    score, ab, g, d = _chain(N, S, True, 2)
    tile = lambda a: np.concatenate([a] * H)                                  # noqa: E731
    key = np.concatenate([np.arange(N) + h * N for h in range(H)])
    assert np.unique(key).size == H * N
    u = sections.philox_uniform(9, np.arange(R)[:, None], key[None, :])
    assert np.unique(u).size == R * H * N
    r = hz.draw_reference(np.arange(H + 1) * N, tile(score), tile(ab), tile(g), tile(d), DZ, SWITCH, R, seed=9, row_key=key)
    x = r["draw_state"].reshape(R, H, N)
    assert not np.array_equal(x[:, 0], x[:, 1]) and not np.array_equal(x[:, 1], x[:, 2])
    one = hz.draw_reference([0, N], score, ab, g, d, DZ, SWITCH, R, seed=9, row_key=np.arange(N) + 2 * N)
    assert np.array_equal(one["draw_state"], x[:, 2])
    # with one key for both, the same evidence gives the same horizon twice: what the convention is there to prevent
    same = hz.draw_reference([0, N, 2 * N], tile(score)[:2 * N], tile(ab)[:2 * N], tile(g)[:2 * N], tile(d)[:2 * N], DZ, SWITCH, R, seed=9,
                             row_key=np.concatenate([np.arange(N)] * 2))
    assert np.array_equal(same["draw_state"][:, :N], same["draw_state"][:, N:])


def test_degenerate_shapes():
    # one sounding, one state: the only path
    r = hz.draw_reference([0, 1], np.zeros((1, 1)), None, [1.0], [0.0], DZ, SWITCH, 4)
    assert np.array_equal(r["draw_state"], np.zeros((4, 1), dtype=np.int32)) and np.array_equal(r["filtered"], [[1.0]])
    # one state and the absent one
    r = hz.draw_reference([0, 3], np.zeros((3, 1)), np.full(3, -50.0), np.ones(3), np.zeros(3), DZ, SWITCH, 50)
    assert r["filtered"].shape == (3, 2) and not r["draw_state"].any()
    # an empty sequence between two others, and no sequence at all
    score, ab, g, d = _chain(4, 3, True, 1)
    cut = hz.draw_reference([0, 1, 1, 4], score, ab, g, d, DZ, SWITCH, 6, seed=3)
    assert cut["margin"].shape == (6, 3) and np.all(np.isinf(cut["margin"][:, 1])) and np.all(np.isfinite(cut["margin"][:, [0, 2]]))
    two = hz.draw_reference([0, 1, 4], score, ab, g, d, DZ, SWITCH, 6, seed=3)
    assert np.array_equal(cut["draw_state"], two["draw_state"])
    none = hz.draw_reference([0], np.zeros((0, 3)), None, [], [], DZ, SWITCH, 2)
    assert none["draw_state"].shape == (2, 0) and none["margin"].shape == (2, 0) and none["filtered"].shape == (0, 3)
    # a state of weight 0 is never drawn
    score = np.zeros((5, 3))
    score[:, 1] = -1000.0                                                     # exp underflows to 0
    z = hz.draw_reference([0, 5], score, None, np.ones(5), np.zeros(5), DZ, SWITCH, 200, seed=4)
    assert not (z["draw_state"] == 1).any() and (z["draw_state"] == 0).any() and (z["draw_state"] == 2).any()


def test_draw_log_scores_are_on_the_scale_of_log_score():
    ptr = np.array([0, 1, 3, 10])
    score, ab, g, d = _chain(10, 5, True, 13)
    t = hz.track_reference(ptr, score, ab, g, d, DZ, SWITCH)
    r = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 300, seed=2)
    states = np.concatenate([t["cell"][None, :], r["draw_state"]])
    ls = hz.draw_log_scores(torch.as_tensor(states), ptr, torch.as_tensor(score), torch.as_tensor(ab), g, d, DZ, SWITCH).numpy()
    assert ls.shape == (301, 3)
    assert np.allclose(ls[0], t["log_score"], rtol=0, atol=1e-12)             # the Viterbi path scores log_score
    assert np.all(ls[1:] <= t["log_score"][None, :] + 1e-12)                  # and no draw scores more
    one = ls[:, 0] - np.where(states[:, 0] < 5, score[0][np.minimum(states[:, 0], 4)], ab[0])
    assert np.allclose(one, 0.0, rtol=0, atol=1e-15)                          # a sequence of one sounding: its node term alone
    # exp(draw_log_score - log_partition) is the path's probability: on the sequence of two soundings the 36 of them sum to 1
    pairs = np.array(list(itertools.product(range(6), repeat=2)))
    full = np.zeros((36, 10), dtype=np.int64)
    full[:, 1:3] = pairs
    p = np.exp(hz.draw_log_scores(torch.as_tensor(full), ptr, torch.as_tensor(score), torch.as_tensor(ab), g, d, DZ, SWITCH).numpy()[:, 1]
               - t["log_partition"][1])
    assert abs(p.sum() - 1.0) <= 1e-12


def test_summaries_of_a_hand_made_case():
    edges = np.arange(5) * 2.0                                                # centres 1, 3, 5, 7
    x, y = np.array([0.0, 10.0, 30.0, 40.0, 60.0, 100.0, 0.0]), np.zeros(7)
    ptr = [0, 6, 7]                                                           # a line of six and a sequence of one sounding
    width = sections.section_widths(x, y, ptr)
    assert np.array_equal(width, [10.0, 15.0, 15.0, 15.0, 30.0, 40.0, 0.0])
    cells = np.array([[0, 1, -1, -1, 2, -1, 3],
                      [-1, -1, -1, -1, -1, -1, -1],
                      [3, 3, 3, 3, 3, 3, -1],
                      [-1, 0, -1, 0, -1, -1, 0]], dtype=np.int32)
    got = {k: v.numpy() for k, v in hz.draw_summary(torch.as_tensor(cells), edges, x, y, ptr).items()}
    ref = hz.draw_summary_reference(cells, edges, x, y, ptr)
    for k in ("present_length", "area_above", "longest_gap"):
        assert got[k].shape == (4, 2) and np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["present_length"], [[55.0, 0.0], [0.0, 0.0], [125.0, 0.0], [30.0, 0.0]])
    assert np.array_equal(got["area_above"], [[10.0 * 1 + 15.0 * 3 + 30.0 * 5, 0.0], [0.0, 0.0], [125.0 * 7, 0.0], [30.0, 0.0]])
    assert np.array_equal(got["longest_gap"], [[40.0, 0.0], [125.0, 0.0], [0.0, 0.0], [70.0, 0.0]])
    # weights in place of the widths, one sequence: a volume
    area = np.array([2.0, 1.0, 1.0, 1.0, 4.0, 1.0, 3.0])
    vol = hz.draw_summary(torch.as_tensor(cells), edges, None, None, None, weights=area)
    assert np.array_equal(vol["area_above"].numpy()[:, 0], [2.0 + 3.0 + 20.0 + 21.0, 0.0, 10.0 * 7, 1.0 + 1.0 + 3.0])
    assert np.array_equal(vol["area_above"].numpy(), hz.draw_summary_reference(cells, edges, None, None, None, weights=area)["area_above"])
    assert vol["longest_gap"].shape == (4, 1) and np.array_equal(vol["longest_gap"].numpy()[:, 0], [2.0, 13.0, 3.0, 5.0])
    # present without a gap from a to b
    assert hz.connected(cells, 0, 1) == 0.5 and hz.connected(cells, 1, 0) == 0.5 and hz.connected(cells, 0, 5) == 0.25
    assert hz.connected(cells, 6, 6) == 0.5 and hz.connected(cells, 2, 2) == 0.25
    with pytest.raises(ValueError, match="draw_cell"):
        hz.draw_summary(torch.as_tensor(cells + 2), edges, x, y, ptr)
    with pytest.raises(ValueError, match="draw_cell"):
        hz.draw_summary(torch.as_tensor(cells).double(), edges, x, y, ptr)
    with pytest.raises(ValueError, match="weights"):
        hz.draw_summary(torch.as_tensor(cells), edges, None, None, None, weights=-area)
    with pytest.raises(ValueError, match="x and y"):
        hz.draw_summary(torch.as_tensor(cells), edges, x[:3], y[:3], ptr)
    with pytest.raises(ValueError, match="connected: a"):
        hz.connected(cells, 7, 0)


def test_refusals_by_message():
    score, ab, g, d = _chain(4, 3, True, 1)
    ok = dict(ptr=[0, 4], score=score, absent_score=ab, g=g, d=d, dz=DZ, switch=SWITCH, n_draws=3)

    def ref(**kw):
        return hz.draw_reference(**{**ok, **kw})

    def dev(**kw):
        a = {**ok, **kw}
        for k in ("score", "absent_score"):
            a[k] = a[k] if a[k] is None or torch.is_tensor(a[k]) or k in kw else torch.as_tensor(a[k])
        return hz.draw(**a)

    for call in (ref, dev):
        with pytest.raises(ValueError, match="n_draws"):
            call(n_draws=0)
        with pytest.raises(ValueError, match="n_draws"):
            call(n_draws=65537)
        with pytest.raises(ValueError, match="seed"):
            call(seed=-1)
        with pytest.raises(ValueError, match="seed"):
            call(seed=2 ** 64)
        with pytest.raises(ValueError, match="row_key"):
            call(row_key=np.arange(3))
        with pytest.raises(ValueError, match="row_key"):
            call(row_key=np.arange(4) * 0.5)
        with pytest.raises(ValueError, match="ptr"):
            call(ptr=[0, 3])
        with pytest.raises(ValueError, match="ptr"):
            call(ptr=[0, 3, 2, 4])
        with pytest.raises(ValueError, match="g and d"):
            call(g=g[:3])
        with pytest.raises(ValueError, match="finite"):
            call(d=np.array([0.0, np.nan, 0.0, 0.0]))
        with pytest.raises(ValueError, match="dz"):
            call(dz=0.0)
        with pytest.raises(ValueError, match="switch"):
            call(switch=-1.0)
    with pytest.raises(ValueError, match="absent_score"):
        ref(absent_score=ab[:3])
    with pytest.raises(ValueError, match="absent_score"):
        dev(absent_score=torch.as_tensor(ab[:3]))
    with pytest.raises(ValueError, match="score must be"):
        ref(score=np.zeros(4))
    with pytest.raises(ValueError, match="score must be"):
        dev(score=torch.zeros((4, 2049), dtype=torch.float64), absent_score=None)
    with pytest.raises(ValueError, match="finite"):
        ref(score=np.full((4, 3), np.inf))
    # the device entry: tensors, float64, and the device last -- there is no host fallback
    from geobipy_amd import _lib
    with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
        dev(score=score)
    with pytest.raises(TypeError, match="float64"):
        dev(score=torch.zeros((4, 3), dtype=torch.float32))
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        dev()
    # the drivers
    ev = torch.ones((4, 6), dtype=torch.float64)
    edges, x = np.arange(7) * 0.5, np.arange(4) * 10.0
    with pytest.raises(ValueError, match="draws"):
        hz.track(ev, x, x, x, edges, draws=-1)
    with pytest.raises(ValueError, match="draws"):
        hz.track(ev, x, x, x, edges, draws=65537)
    with pytest.raises(ValueError, match="seed"):
        hz.track(ev, x, x, x, edges, draws=2, seed=-3)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        hz.track(ev, x, x, x, edges, draws=2)


def test_c_entry_refuses_bad_arguments():
    from geobipy_amd import _lib
    lib = _lib.load()                                                         # (the suite builds it: a library that does not load is a failure)
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(L=2, ptr=p, total=5, max_n=3, S=4, dz=0.5, score=p, absent=None, g=p, d=p, switch=1.0, row_key=None, seed=0, n_draws=3, filtered=p,
             scale=p, draw_state=p):
        return lib.gbp_horizon_draw(L, ptr, total, max_n, S, dz, score, absent, g, d, switch, row_key, seed, n_draws, filtered, scale, draw_state, None)

    err = lib.gbp_last_error
    # every one of these is refused before anything touches a device
    assert call(L=-1) == INVALID and b"gbp_horizon_draw" in err() and b"L must" in err()
    assert call(S=0) == INVALID and call(S=2049) == INVALID and b"gbp_horizon_draw" in err() and b"S must" in err()
    assert call(n_draws=0) == INVALID and call(n_draws=65537) == INVALID and b"n_draws must" in err()
    assert call(dz=0.0) == INVALID and call(dz=float("nan")) == INVALID and b"dz" in err()
    assert call(switch=-0.5) == INVALID and call(switch=float("nan")) == INVALID and b"switch" in err()
    for name in ("ptr", "score", "g", "d", "filtered", "scale", "draw_state"):
        assert call(**{name: None}) == INVALID, name
        assert b"gbp_horizon_draw" in err() and b"NULL" in err(), name
    assert call(total=-1) == INVALID and call(max_n=6) == INVALID and call(total=7) == INVALID and b"total_n" in err()
    assert call(L=1, total=1 << 60, max_n=1 << 30) == INVALID and b"total_n" in err()
    assert call(L=2 ** 31 - 1, total=2 ** 50, max_n=2 ** 20, S=2048) == INVALID and b"out of range" in err()
    assert call(L=2 ** 31 - 1, total=2 ** 47, max_n=2 ** 17, S=1, n_draws=65536) == INVALID and b"n_draws * total_n" in err()
    # no sequences, or only empty ones: no launch, whatever the pointers -- but the sizes are still checked
    assert call(L=0, ptr=None, total=0, max_n=0, score=None, g=None, d=None, filtered=None, scale=None, draw_state=None) == 0
    assert call(L=3, ptr=None, total=0, max_n=0, score=None, g=None, d=None, filtered=None, scale=None, draw_state=None) == 0
    assert call(L=0, S=0) == INVALID and call(L=0, n_draws=0) == INVALID


def test_header_include_order_and_build_list():
    header = open(os.path.join(ROOT, "include", "geobipy_amd.h")).read()
    m = re.search(r"gbp_status gbp_horizon_draw\((.*?)\);", header, re.S)
    assert m is not None and len(m.group(1).split(",")) == 18
    from geobipy_amd import _lib
    assert len(_lib.SIGNATURES["gbp_horizon_draw"][1]) == 18
    src = open(os.path.join(build.CSRC, "gbp_fdem.hip")).read()
    order = re.findall(r'#include "(gbp_[a-z_]+\.h)"', src)
    assert order.index("gbp_horizon_graph.h") < order.index("gbp_horizon_draw.h") < order.index("gbp_section_graph_draw.h")
    assert order.index("gbp_horizon.h") < order.index("gbp_horizon_draw.h") and order.count("gbp_horizon_draw.h") == 1
    assert "gbp_horizon_draw.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "gbp_horizon_draw.h"))
    m = re.search(r'extern "C" gbp_status gbp_horizon_draw\((.*?)\)\s*\{', src, re.S)
    assert m is not None and len(m.group(1).split(",")) == 18
    kernels = open(os.path.join(build.CSRC, "gbp_horizon_draw.h")).read()
    assert "namespace horizon_draw" in kernels and "atomic" not in kernels.split("#pragma once")[1].replace("No atomics", "")


def test_command_line_parser():
    a = hz.parse_args(["out", "--between", "5", "40", "--draws", "16", "--seed", "3"])
    assert a.draws == 16 and a.seed == 3 and a.spatial is None
    a = hz.parse_args(["out", "--between", "5", "40"])
    assert a.draws == 0 and a.seed == 0
    for bad in (["out", "--between", "5", "40", "--draws", "-1"], ["out", "--between", "5", "40", "--draws", "65537"],
                ["out", "--between", "5", "40", "--seed", "3"], ["out", "--between", "5", "40", "--draws", "2", "--seed", "-1"]):
        with pytest.raises(SystemExit):
            hz.parse_args(bad)


# ---- across lines: the rule of the line-blocked Gibbs sampler (horizons.graph_draw_reference) ------------------------------------------

from test_horizon_graph import brute_force, horizon_inputs, planted_horizon, PER_LINE, DECOY_CELLS  # noqa: E402
from test_section_draws import R_STAT, worst_z  # noqa: E402
from test_spatial_sections import lattice_graph, star_graph  # noqa: E402

LATTICE_SEED, LATTICE_SWEEPS = 4, 6


def chain_as_graph(ptr, g, d):
    """The steps of the sequences of ``ptr`` as the edges of a graph without cross edges: eu, ev, g, d [E]."""
    last = np.zeros(int(ptr[-1]), dtype=bool)
    last[np.asarray(ptr[1:])[np.diff(ptr) > 0] - 1] = True
    eu = np.flatnonzero(~last)
    return eu, eu + 1, np.asarray(g)[eu], np.asarray(d)[eu]


def lattice_case():
    """The 2 x 3 lattice of tests/test_horizon_graph.py (3 cells + absent: 4^6 configurations) as two lines of three."""
    rng = np.random.default_rng(2)
    eu, ev, N = lattice_graph(2, 3)
    S, switch = 3, 1.5
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, True, slope=0.8)
    return eu, ev, g, d, dz, switch, score, ab, np.array([0, 3, 6])


def exact_pairs(every, SA, N, a, b):
    """The exact pair marginal [SA, SA] of soundings a, b from the log scores of every configuration (itertools.product order)."""
    cfgs = np.array(list(itertools.product(range(SA), repeat=N)))
    p = np.exp(every - every.max())
    p = p / p.sum()
    pair = np.zeros((SA, SA))
    np.add.at(pair, (cfgs[:, a], cfgs[:, b]), p)
    return pair


def marginal_z(draw_state, marginal, R, least=8):
    counts = np.stack([np.bincount(draw_state[:, s], minlength=marginal.shape[1]) for s in range(marginal.shape[0])])
    return worst_z(counts, np.asarray(marginal, dtype=np.float64), R, least)[0]


def check_lattice(draw_state, what, R=R_STAT):
    """Single and pair marginals of the lattice against the enumeration in long double, within 5 sigma."""
    eu, ev, g, d, dz, switch, score, ab, _ = lattice_case()
    want, _, _, every = brute_force(eu, ev, g, d, dz, switch, score, ab)
    z = marginal_z(draw_state, want, R)
    worst_pair = 0.0
    for a, b in ((1, 4), (0, 5), (0, 1)):                                     # a cross edge, two corners, a step
        pair = exact_pairs(every, 4, 6, a, b)
        counts = np.zeros((4, 4))
        np.add.at(counts, (draw_state[:, a], draw_state[:, b]), 1.0)
        cells = (R * pair >= 30.0) & (pair < 1.0)
        assert cells.sum() >= 2
        worst_pair = max(worst_pair, float((np.abs(counts[cells] - R * pair[cells]) / np.sqrt(R * pair[cells] * (1.0 - pair[cells]))).max()))
    print("%s: worst |z| of the marginals %.2f, of the pairs %.2f" % (what, z, worst_pair))
    return z, worst_pair


def test_graph_rule_without_cross_edges_starts_as_draw_reference():
    ptr, S = np.array([0, 5, 5, 6, 12]), 5
    score, ab, g, d = _chain(12, S, True, 6)
    eu, ev, ge, de = chain_as_graph(ptr, g, d)
    key = (np.arange(12) * 7 + 2 ** 33).astype(np.int64)
    want = hz.draw_reference(ptr, score, ab, g, d, DZ, SWITCH, 300, seed=3, row_key=key)
    got = hz.graph_draw_reference(eu, ev, ge, de, DZ, SWITCH, score, ab, ptr, 300, seed=3, sweeps=0, row_key=key)
    assert got["draw_state"].dtype == np.int32 and np.array_equal(got["draw_state"], want["draw_state"])
    for l in (0, 2, 3):
        assert np.array_equal(got["margin"][:, ptr[l]:ptr[l + 1]], np.repeat(want["margin"][:, l:l + 1], ptr[l + 1] - ptr[l], axis=1))
    assert np.array_equal(got["filtered"][7], want["filtered"]) and got["filtered"].shape == (300, 12, S + 1)
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    assert colour.tolist() == [0, 0, 0, 0] and n_colours == 1
    # sweeps redraw every line from the same law: the marginals stay the chain's, the draws change with the sweep
    three = hz.graph_draw_reference(eu, ev, ge, de, DZ, SWITCH, score, ab, ptr, R_STAT, seed=3, sweeps=3, row_key=key)
    assert not np.array_equal(three["draw_state"][:300], want["draw_state"])
    ld = hz.track_reference(ptr[[0, 1, 3, 4]], score, ab, g, d, DZ, SWITCH, dtype=np.longdouble)["marginal"].astype(np.float64)
    assert marginal_z(three["draw_state"], ld, R_STAT) <= 5.0
    assert np.all(three["margin"][:300] <= got["margin"])


def test_the_lattice_reaches_the_exact_joint_and_the_start_does_not():
    eu, ev, g, d, dz, switch, score, ab, ptr = lattice_case()
    colour, n_colours = sections.line_colours(eu, ev, ptr)
    assert colour.tolist() == [0, 1] and n_colours == 2
    start = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, R_STAT, seed=LATTICE_SEED, sweeps=0)
    z0, p0 = check_lattice(start["draw_state"], "lattice, the line-alone start")
    assert max(z0, p0) > 5.0                                                  # a scheme that ignores the cross edges is seen
    for T in (LATTICE_SWEEPS, 2 * LATTICE_SWEEPS):
        out = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, R_STAT, seed=LATTICE_SEED, sweeps=T)
        z, zp = check_lattice(out["draw_state"], "lattice, %d sweeps" % T)
        assert z <= 5.0 and zp <= 5.0
        assert out["draw_state"].min() >= 0 and out["draw_state"].max() <= 3


def test_singletons_on_the_star_are_single_site_gibbs():
    rng = np.random.default_rng(1)
    eu, ev, _ = star_graph()
    N, S, switch = 5, 3, 1.5
    score, ab, g, d, dz = horizon_inputs(rng, eu, ev, N, S, True, slope=0.8)
    want, _, _, _ = brute_force(eu, ev, g, d, dz, switch, score, ab)
    out = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, np.arange(N + 1), R_STAT, seed=5, sweeps=12)
    z = marginal_z(out["draw_state"], want, R_STAT)
    print("star as singletons, 12 sweeps: worst |z| = %.2f" % z)
    assert z <= 5.0
    assert sections.line_colours(eu, ev, np.arange(N + 1))[1] == 2


def test_graph_rule_continuation_and_independence_of_R():
    eu, ev, g, d, dz, switch, score, ab, ptr = lattice_case()
    key = np.arange(6, dtype=np.int64) + (7 << 32)
    whole = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, 40, seed=9, sweeps=5, row_key=key)
    few = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, 7, seed=9, sweeps=5, row_key=key)
    assert np.array_equal(few["draw_state"], whole["draw_state"][:7]) and np.array_equal(few["filtered"], whole["filtered"][:7])
    half = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, 40, seed=9, sweeps=2, row_key=key)
    rest = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, 40, seed=9, sweeps=5, row_key=key, state=half["draw_state"], first_sweep=3)
    assert np.array_equal(rest["draw_state"], whole["draw_state"]) and np.array_equal(rest["filtered"], whole["filtered"])
    assert np.all(np.minimum(half["margin"], rest["margin"]) == whole["margin"])
    other = hz.graph_draw_reference(eu, ev, g, d, dz, switch, score, ab, ptr, 40, seed=9, sweeps=5)
    assert not np.array_equal(other["draw_state"], whole["draw_state"])


def test_the_planted_lines_draw_the_planted_horizon_on_the_graph():
    """The planted lines of DESIGN.md 3.33: alone, the middle line's draws sit on the decoy; on the graph the planted cell holds more
    than half of them."""
    evidence, x, y, surface, edges, ptr, cell = planted_horizon()
    middle = np.arange(PER_LINE, 2 * PER_LINE)
    score, _ = hz.evidence_scores(evidence)
    eu, ev, _, _ = sections.neighbours(x, y, ptr, None, max_distance=150.0)
    g, d, _ = hz.graph_steps(x, y, surface, eu, ev)
    R = 64
    alone = hz.graph_draw_reference(eu, ev, g, d, 1.0, 4.6, score, None, ptr, R, seed=1, sweeps=0)["draw_state"]
    graph = hz.graph_draw_reference(eu, ev, g, d, 1.0, 4.6, score, None, ptr, R, seed=1, sweeps=8)["draw_state"]
    on_alone = float((alone[:, middle] == cell[middle][None, :]).mean())
    on_graph = float((graph[:, middle] == cell[middle][None, :]).mean())
    print("planted cell of the middle line: %.3f of the line-alone draws, %.3f of the graph draws; decoy: %.3f / %.3f"
          % (on_alone, on_graph, float((alone[:, middle] == cell[middle] + DECOY_CELLS).mean()), float((graph[:, middle] == cell[middle] + DECOY_CELLS).mean())))
    assert on_alone < on_graph and on_graph > 0.5


def test_graph_refusals_by_message():
    eu, ev, g, d, dz, switch, score, ab, ptr = lattice_case()
    ok = dict(eu=eu, ev=ev, g=g, d=d, dz=dz, switch=switch, score=score, absent_score=ab, ptr=ptr, n_draws=3)

    def ref(**kw):
        return hz.graph_draw_reference(**{**ok, **kw})

    def dev(**kw):
        a = {**ok, **kw}
        for k in ("score", "absent_score"):
            a[k] = a[k] if a[k] is None or torch.is_tensor(a[k]) or k in kw else torch.as_tensor(a[k])
        return hz.graph_draw(**a)

    for call in (ref, dev):
        with pytest.raises(ValueError, match="n_draws"):
            call(n_draws=0)
        with pytest.raises(ValueError, match="sweeps"):
            call(sweeps=-1)
        with pytest.raises(ValueError, match="sweeps"):
            call(sweeps=65536)
        with pytest.raises(ValueError, match="first_sweep"):
            call(sweeps=2, first_sweep=3, state=np.zeros((3, 6), dtype=np.int32))
        with pytest.raises(ValueError, match="goes with first_sweep"):
            call(first_sweep=1)
        with pytest.raises(ValueError, match="goes with first_sweep"):
            call(state=np.zeros((3, 6), dtype=np.int32))
        with pytest.raises(ValueError, match="state"):
            call(first_sweep=1, state=np.zeros((2, 6), dtype=np.int32))
        with pytest.raises(ValueError, match="state"):
            call(first_sweep=1, state=np.full((3, 6), 4, dtype=np.int32))
        with pytest.raises(ValueError, match="seed"):
            call(seed=-1)
        with pytest.raises(ValueError, match="row_key"):
            call(row_key=np.arange(5))
        with pytest.raises(ValueError, match="is not a step"):
            call(ptr=[0, 6])                                                   # (0, 3) would lie inside the one sequence
        with pytest.raises(ValueError, match="is missing"):
            call(eu=eu[1:], ev=ev[1:], g=g[1:], d=d[1:])                        # the step 0 -> 1 is gone
        with pytest.raises(ValueError, match="ptr"):
            call(ptr=[0, 3, 5])
        with pytest.raises(ValueError, match="g and d"):
            call(g=g[:3])
        with pytest.raises(ValueError, match="dz"):
            call(dz=-1.0)
    with pytest.raises(ValueError, match="block"):
        dev(block=0)
    with pytest.raises(ValueError, match="budget_bytes"):
        dev(budget_bytes=0)
    from geobipy_amd import _lib
    with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
        dev(score=score)
    with pytest.raises(TypeError, match="float64"):
        dev(score=torch.zeros((6, 3), dtype=torch.float32))
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        dev()
    ev_t = torch.ones((4, 6), dtype=torch.float64)
    edges, x = np.arange(7) * 0.5, np.arange(4) * 10.0
    with pytest.raises(ValueError, match="draws"):
        hz.spatial(ev_t, x, x, x, edges, max_distance=15.0, draws=-1)
    with pytest.raises(ValueError, match="draw_sweeps"):
        hz.spatial(ev_t, x, x, x, edges, max_distance=15.0, draws=2, draw_sweeps=-1)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        hz.spatial(ev_t, x, x, x, edges, max_distance=15.0, draws=2)


def test_graph_entry_refuses_bad_arguments_and_is_declared():
    from geobipy_amd import _lib
    header = open(os.path.join(ROOT, "include", "geobipy_amd.h")).read()
    m = re.search(r"gbp_status gbp_horizon_graph_draw\((.*?)\);", header, re.S)
    assert m is not None and len(m.group(1).split(",")) == 29 and len(_lib.SIGNATURES["gbp_horizon_graph_draw"][1]) == 29
    src = open(os.path.join(build.CSRC, "gbp_fdem.hip")).read()
    m = re.search(r'extern "C" gbp_status gbp_horizon_graph_draw\((.*?)\)\s*\{', src, re.S)
    assert m is not None and len(m.group(1).split(",")) == 29
    lib = _lib.load()
    INVALID = -1
    buf = (ctypes.c_byte * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(N=6, E=7, S=3, has_absent=1, dz=0.5, switch=1.0, eu=p, ev=p, score=p, g=p, d=p, L=2, ptr=p, step_edge=p, cross_ptr=p, cross_edge=p,
             n_colours=2, colour_ptr=p, colour_line=p, row_key=None, seed=0, n_draws=3, first_draw=0, first_sweep=0, sweeps=2, alpha=p, scale=p,
             draw_state=p):
        return lib.gbp_horizon_graph_draw(N, E, S, has_absent, dz, switch, eu, ev, score, g, d, L, ptr, step_edge, cross_ptr, cross_edge, n_colours,
                                          colour_ptr, colour_line, row_key, seed, n_draws, first_draw, first_sweep, sweeps, alpha, scale, draw_state, None)

    err = lib.gbp_last_error
    for kw, word in ((dict(N=-1), b"N must"), (dict(S=0), b"S must"), (dict(S=2049), b"S must"), (dict(has_absent=2), b"has_absent"),
                     (dict(dz=0.0), b"dz"), (dict(switch=-1.0), b"switch"), (dict(E=-1), b"E must"), (dict(L=-1), b"L must"), (dict(L=0), b"L >= 1"),
                     (dict(n_draws=0), b"n_draws must"), (dict(n_draws=65537), b"n_draws must"), (dict(first_draw=-1), b"first_draw"),
                     (dict(first_draw=65534), b"first_draw"), (dict(first_sweep=-1), b"sweeps"), (dict(first_sweep=3), b"sweeps"),
                     (dict(sweeps=65536), b"sweeps"), (dict(n_colours=0), b"colour lists must cover"), (dict(n_colours=3), b"colour lists must cover"),
                     # (n_draws * N * SA doubles fit 63 bits under the limits above; the grid of the conditioned filter is what can overflow)
                     (dict(L=2 ** 20, n_colours=1, n_draws=65536), b"L * n_draws out of range")):
        assert call(**kw) == INVALID and b"gbp_horizon_graph_draw" in err() and word in err(), (kw, err())
    for name in ("score", "ptr", "step_edge", "cross_ptr", "colour_ptr", "colour_line", "alpha", "scale", "draw_state", "eu", "ev", "g", "d", "cross_edge"):
        assert call(**{name: None}) == INVALID and b"gbp_horizon_graph_draw" in err() and b"NULL" in err(), name
    assert call(N=0, E=0, L=0, score=None, ptr=None, alpha=None, scale=None, draw_state=None) == 0
    assert call(N=0, E=0, L=0, S=0) == INVALID


def test_command_line_takes_draws_on_the_graph():
    a = hz.parse_args(["out", "--between", "5", "40", "--spatial", "150", "--draws", "16", "--seed", "3", "--draw-sweeps", "4"])
    assert a.draws == 16 and a.seed == 3 and a.draw_sweeps == 4 and a.spatial == 150.0
    a = hz.parse_args(["out", "--between", "5", "40", "--spatial", "150", "--draws", "16"])
    assert a.draw_sweeps is None                                              # (the default of spatial: 8)
    for bad in (["out", "--between", "5", "40", "--draws", "2", "--draw-sweeps", "4"], ["out", "--between", "5", "40", "--spatial", "150", "--draw-sweeps", "4"],
                ["out", "--between", "5", "40", "--spatial", "150", "--draws", "2", "--draw-sweeps", "-1"],
                ["out", "--between", "5", "40", "--spatial", "150", "--draws", "2", "--draw-sweeps", "65536"]):
        with pytest.raises(SystemExit):
            hz.parse_args(bad)
