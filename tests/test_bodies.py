"""Connected bodies of joint realisations, host side (geobipy_amd.bodies): the rule ``label_reference`` held to scipy
(``ndimage.label`` with 4-connectivity on a line graph, ``sparse.csgraph.connected_components`` on random graphs, both relabelled to the
smallest index of every body), hand-made cases with their labels written out, the quantised measure against a long-double sum, the
torch reductions on top of the labels, and every refusal by its message.  The device is held to the same rule in test_bodies_gpu.py."""
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, bodies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line_edges(S):
    return np.arange(S - 1), np.arange(1, S)


def smallest_index(component, member):
    """Labels of any numbering -> the rule's: the smallest linear index of every component, -1 outside ``member``."""
    comp, flat = np.asarray(component).reshape(-1), np.asarray(member).reshape(-1)
    out = np.full(comp.size, -1, dtype=np.int32)
    first = {}
    for i in np.flatnonzero(flat):
        out[i] = first.setdefault(int(comp[i]), int(i))
    return out.reshape(np.asarray(member).shape)


def cells_of(label):
    flat = label.reshape(-1)
    out = np.zeros(flat.size, dtype=np.int32)
    np.add.at(out, flat[flat >= 0], 1)
    return out.reshape(label.shape)


def serpentine(S, C):
    """One body: every even sounding is a full bar, the odd ones join the bars at the bottom and at the top in turn."""
    m = np.zeros((S, C), dtype=bool)
    m[0::2] = True
    m[1::4, C - 1] = True
    m[3::4, 0] = True
    return m


def as_lab(ref, group_ptr):
    """A result of ``label_reference`` ([R, S, C]) as ``label`` would return it, on the host."""
    lab = {name: torch.as_tensor(v) for name, v in ref.items() if name != "unit"}
    if "unit" in ref:
        lab["unit"] = ref["unit"]
    lab["group_ptr"] = np.asarray(group_ptr, dtype=np.int64)
    return lab


# ---- the rule against scipy -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,C,density,seed", [(1, 1, 0.5, 0), (1, 17, 0.6, 1), (9, 1, 0.6, 2), (12, 9, 0.3, 3), (20, 31, 0.59, 4), (20, 31, 0.9, 5),
                                              (33, 7, 0.59, 6)])
def test_the_rule_on_a_line_is_ndimage_label(S, C, density, seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    member = np.random.default_rng(seed).random((S, C)) < density
    eu, ev = line_edges(S)
    got = bodies.label_reference(member, eu, ev)
    comp, n = ndimage.label(member, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    want = smallest_index(comp, member)
    assert got["label"].dtype == np.int32 and got["cells"].dtype == np.int32
    assert np.array_equal(got["label"], want) and np.array_equal(got["cells"], cells_of(want))
    assert int((got["cells"] > 0).sum()) == n


@pytest.mark.parametrize("S,C,E,density,seed", [(6, 4, 5, 0.6, 0), (15, 5, 12, 0.5, 1), (15, 5, 40, 0.4, 2), (30, 3, 25, 0.7, 3), (8, 11, 0, 0.6, 4)])
def test_the_rule_on_random_graphs_is_csgraph(S, C, E, density, seed):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(seed)
    member = rng.random((2, S, C)) < density
    eu, ev = rng.integers(0, S, E), rng.integers(0, S, E)                      # any direction, repeats and self-loops included
    got = bodies.label_reference(member, eu, ev)
    for r in range(2):
        m = member[r]
        idx = np.arange(S * C).reshape(S, C)
        i = [idx[:, :-1][m[:, :-1] & m[:, 1:]]] + [idx[u][m[u] & m[v]] for u, v in zip(eu, ev)]
        j = [idx[:, 1:][m[:, :-1] & m[:, 1:]]] + [idx[v][m[u] & m[v]] for u, v in zip(eu, ev)]
        i, j = np.concatenate(i), np.concatenate(j)
        graph = sparse.coo_matrix((np.ones(i.size), (i, j)), shape=(S * C, S * C))
        _, comp = connected_components(graph, directed=False)
        want = smallest_index(comp.reshape(S, C), m)
        assert np.array_equal(got["label"][r], want) and np.array_equal(got["cells"][r], cells_of(want))


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------

def test_hand_made_cases_with_their_labels_written_out():
    eu, ev = line_edges(5)
    snake = bodies.label_reference(serpentine(5, 3), eu, ev)
    assert np.array_equal(snake["label"], [[0, 0, 0], [-1, -1, 0], [0, 0, 0], [0, -1, -1], [0, 0, 0]])
    assert snake["cells"][0, 0] == 11 and snake["cells"].sum() == 11
    comb = np.zeros((5, 3), dtype=bool)
    comb[0::2] = True
    comb[:, 0] = True                                                          # the back of the comb
    assert np.array_equal(bodies.label_reference(comb, eu, ev)["label"], [[0, 0, 0], [0, -1, -1], [0, 0, 0], [0, -1, -1], [0, 0, 0]])
    comb[1::2, 0] = False                                                      # the teeth alone
    teeth = bodies.label_reference(comb, eu, ev)
    assert np.array_equal(teeth["label"], [[0, 0, 0], [-1, -1, -1], [6, 6, 6], [-1, -1, -1], [12, 12, 12]])
    assert np.array_equal(teeth["cells"].reshape(-1)[[0, 6, 12]], [3, 3, 3]) and teeth["cells"].sum() == 9
    board = (np.add.outer(np.arange(5), np.arange(3)) % 2) == 0
    own = bodies.label_reference(board, eu, ev)
    assert np.array_equal(own["label"], np.where(board, np.arange(15).reshape(5, 3), -1)) and np.array_equal(own["cells"], board.astype(np.int32))
    full = bodies.label_reference(np.ones((5, 3), dtype=bool), eu, ev)
    assert np.all(full["label"] == 0) and full["cells"][0, 0] == 15 and full["cells"].sum() == 15
    none = bodies.label_reference(np.zeros((5, 3), dtype=bool), eu, ev)
    assert np.all(none["label"] == -1) and np.all(none["cells"] == 0)


def test_membership_nan_infinities_and_equal_bounds():
    v = np.array([[np.nan, 1.0, 2.0, np.inf, -np.inf, 3.0]])
    assert np.array_equal(bodies.member_reference(v, 1.0, 2.0), [[False, True, True, False, False, False]])
    assert np.array_equal(bodies.member_reference(v, -np.inf, 2.0), [[False, True, True, False, True, False]])
    assert np.array_equal(bodies.member_reference(v, 2.0, np.inf), [[False, False, True, True, False, True]])
    assert np.array_equal(bodies.member_reference(v, -np.inf, np.inf), [[False, True, True, True, True, True]])
    assert np.array_equal(bodies.member_reference(v, 2.0, 2.0), [[False, False, True, False, False, False]])
    assert not bodies.member_reference(v, 2.0, 1.0).any()
    lab = bodies.label_reference(bodies.member_reference(v, -np.inf, np.inf), [], [])
    assert np.array_equal(lab["label"], [[-1, 1, 1, 1, 1, 1]])


def test_edges_both_ways_twice_isolated_soundings_and_empty_groups():
    member = np.ones((4, 2), dtype=bool)
    once = bodies.label_reference(member, [0], [1])
    often = bodies.label_reference(member, [0, 1, 0, 1], [1, 0, 1, 0])
    assert np.array_equal(once["label"], often["label"]) and np.array_equal(once["cells"], often["cells"])
    assert np.array_equal(once["label"], [[0, 0], [0, 0], [4, 4], [6, 6]])    # soundings 2 and 3 are isolated: a body each
    assert np.array_equal(bodies.default_groups(np.array([0]), np.array([1]), 4), [0, 2, 3, 4])
    assert np.array_equal(bodies.default_groups(np.array([0]), np.array([2]), 4), [0, 4])      # a piece that is no range: one group
    assert np.array_equal(bodies.default_groups(np.zeros(0, dtype=int), np.zeros(0, dtype=int), 0), [0])
    p, gu = bodies.check_groups([0, 2, 2, 4], np.array([3, 0]), np.array([2, 1]), 4)          # the middle group is empty
    assert np.array_equal(p, [0, 2, 2, 4]) and np.array_equal(gu, [2, 0])
    with pytest.raises(ValueError, match="an edge joins two groups"):
        bodies.check_groups([0, 2, 2, 4], np.array([1]), np.array([2]), 4)
    with pytest.raises(ValueError, match="ptr must start at 0"):
        bodies.check_groups([0, 2, 3], np.array([0]), np.array([1]), 4)


# ---- the measure ----------------------------------------------------------------------------------------------------------------------

def test_the_quantised_measure_against_the_long_double_sum():
    rng = np.random.default_rng(7)
    S, C = 25, 40
    member = rng.random((3, S, C)) < 0.62
    a, t = rng.uniform(5.0, 60.0, S), np.diff(np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 12.0, C))]))
    a[3], t[5] = 0.0, 0.0                                                      # a sounding and a cell that stand for nothing
    eu, ev = line_edges(S)
    ref = bodies.label_reference(member, eu, ev, a=a, t=t)
    q, unit = bodies.quantise(a, t)
    assert unit == ref["unit"] == (a.max() * t.max()) * 2.0 ** -30 and q.max() == 2 ** 30 and q.min() == 0 and q.dtype == np.int64
    assert np.array_equal(q, np.rint((a[:, None] * t[None, :]) / unit).astype(np.int64))
    exact = a.astype(np.longdouble)[:, None] * t.astype(np.longdouble)[None, :]
    worst = 0.0
    for r in range(3):
        roots = np.flatnonzero(ref["cells"][r].reshape(-1))
        assert roots.size > 3
        for root in roots:
            body = ref["label"][r] == root
            assert ref["measure_q"][r].reshape(-1)[root] == q[body].sum()
            err = abs(float(np.longdouble(ref["measure_q"][r].reshape(-1)[root]) * np.longdouble(unit) - exact[body].sum()))
            worst = max(worst, err / (body.sum() * unit / 2.0))
            assert err <= body.sum() * unit / 2.0
        assert np.all(ref["measure_q"][r].reshape(-1)[np.setdiff1d(np.arange(S * C), roots)] == 0)
    print("the quantised measure: at most %.3f of cells * unit / 2 from the long-double sum" % worst)
    assert np.array_equal(ref["measure"], ref["measure_q"].astype(np.float64) * unit)


# ---- the reductions on top of the labels ----------------------------------------------------------------------------------------------

def two_bodies():
    """A section of 6 soundings and 4 columns: a shallow body under soundings 0 .. 2 and one of equal size under 3 .. 5, a column apart;
    in the second realisation sounding 3 joins them."""
    m = np.zeros((2, 6, 4), dtype=bool)
    m[:, 0:3, 0:2] = True
    m[:, 3:6, 2:4] = True
    m[1, 3, :] = True
    return m


def test_summary_counts_sizes_and_breaks_ties_by_the_smallest_root():
    m = two_bodies()
    eu, ev = line_edges(6)
    a, t = np.full(6, 10.0), np.full(4, 2.0)
    lab = as_lab(bodies.label_reference(m, eu, ev, a=a, t=t), [0, 6])
    s = bodies.summary(lab)
    assert s["n_bodies"].tolist() == [[2], [1]]
    assert s["largest_root"].tolist() == [[0], [0]]                            # a tie of 6 cells against 6: the smaller root
    assert s["largest_cells"].tolist() == [[6], [14]]
    assert s["largest_measure"].tolist() == [[120.0], [280.0]] and s["member_measure"].tolist() == [[240.0], [280.0]]
    t2 = np.array([2.0, 2.0, 3.0, 3.0])                                        # the deeper body is larger by measure, equal by cells
    by_measure = bodies.summary(as_lab(bodies.label_reference(m[:1], eu, ev, a=a, t=t2), [0, 6]))
    assert by_measure["largest_root"].tolist() == [[14]] and by_measure["largest_cells"].tolist() == [[6]]
    assert abs(by_measure["largest_measure"][0, 0].item() - 180.0) <= 6 * lab["unit"]
    by_cells = bodies.summary(as_lab(bodies.label_reference(m[:1], eu, ev), [0, 6]))
    assert by_cells["largest_root"].tolist() == [[0]] and "largest_measure" not in by_cells and "member_measure" not in by_cells
    groups = bodies.summary(as_lab(bodies.label_reference(m[:1], eu[[0, 1, 3, 4]], ev[[0, 1, 3, 4]], a=a, t=t), [0, 3, 3, 6]))
    assert groups["n_bodies"].tolist() == [[1, 0, 1]] and groups["largest_root"].tolist() == [[0, -1, 14]]
    assert groups["largest_cells"].tolist() == [[6, 0, 6]] and groups["member_measure"].tolist() == [[120.0, 0.0, 120.0]]
    large = bodies.summary(lab, min_cells=7)
    assert large["n_bodies"].tolist() == [[0], [1]] and large["largest_root"].tolist() == [[-1], [0]] and large["member_measure"].tolist() == [[0.0], [280.0]]
    with pytest.raises(ValueError, match="min_cells must be an integer"):
        bodies.summary(lab, min_cells=0)


def test_connected_and_reach_on_a_two_body_section():
    m = two_bodies()
    eu, ev = line_edges(6)
    lab = as_lab(bodies.label_reference(m, eu, ev, a=np.full(6, 10.0), t=np.full(4, 2.0)), [0, 6])
    c = bodies.connected(lab, [(0, 0), (0, 0), (0, 3)], [(5, 3), (2, 1), (5, 3)])
    assert c["connected"].tolist() == [[False, True, False], [True, True, False]] and c["probability"].tolist() == [0.5, 1.0, 0.0]
    r = bodies.reach(lab, [(0, 0), (0, 3)])
    assert r["share"].shape == (2, 6, 4) and r["seed_member"].tolist() == [1.0, 0.0] and not r["share"][1].any()
    want = (m[0] & (np.arange(6)[:, None] < 3)) * 0.5 + m[1] * 0.5
    assert np.array_equal(r["share"][0].numpy(), want)
    assert r["cells"].tolist() == [[6, 0], [14, 0]] and r["measure"].tolist() == [[120.0, 0.0], [280.0, 0.0]]
    for bad in ([(6, 0)], [(0, 4)], [(-1, 0)], [0, 1], [(0.5, 1.0)]):
        with pytest.raises(ValueError, match="bodies.reach"):
            bodies.reach(lab, bad)
    with pytest.raises(ValueError, match="one pair per question"):
        bodies.connected(lab, [(0, 0)], [(1, 1), (2, 2)])


def test_sounding_areas_sum_to_the_covered_area():
    index = torch.tensor([[0, 0, 1, -1], [0, 2, 2, -1], [2, 2, 2, 1]], dtype=torch.int32)
    plan = types.SimpleNamespace(index=index, n_soundings=4, x_edges=np.arange(5) * 25.0, y_edges=np.arange(4) * 10.0)
    area = bodies.sounding_areas(plan)
    assert area.dtype == np.float64 and area.tolist() == [750.0, 500.0, 1250.0, 0.0]
    assert area.sum() == int((index >= 0).sum()) * 250.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_by_message():
    v = torch.zeros((2, 4, 3), dtype=torch.float64)
    eu, ev = line_edges(4)
    ok = dict(raster=v, lo=0.0, hi=1.0, eu=eu, ev=ev)

    def refuse(kind, message, **kw):
        with pytest.raises(kind, match=message):
            bodies.label(**dict(ok, **kw))

    refuse(_lib.NativeLibraryError, "takes torch tensors on the device", raster=v.numpy())
    refuse(ValueError, r"raster is \[R, S, C\]", raster=v[0])
    refuse(ValueError, r"raster is \[R, S, C\]", raster=v[:, :, :0])
    refuse(ValueError, "at most 65536 realisations, 4096 columns", raster=torch.zeros((1, 1, 4097), dtype=torch.float64))
    refuse(TypeError, "raster is float64", raster=v.float())
    refuse(ValueError, "lo must be a number, not NaN", lo=float("nan"))
    refuse(ValueError, "hi must be a number, not NaN", hi=None)
    refuse(ValueError, "one entry per edge", ev=ev[:-1])
    refuse(TypeError, "eu and ev are integers", eu=eu.astype(np.float64))
    refuse(ValueError, "outside 0 .. S - 1", ev=ev + 1)
    refuse(ValueError, "outside 0 .. S - 1", eu=eu - 1)
    refuse(ValueError, "a and t are given together", a=np.ones(4))
    refuse(ValueError, "a holds one entry per sounding", a=np.ones(3), t=np.ones(3))
    refuse(ValueError, "a holds one entry per sounding", a=np.ones(4), t=np.ones(4))
    refuse(ValueError, "a and t must be finite and >= 0", a=np.array([1.0, -1.0, 1.0, 1.0]), t=np.ones(3))
    refuse(ValueError, "a and t must be finite and >= 0", a=np.ones(4), t=np.array([1.0, np.inf, 1.0]))
    refuse(ValueError, "unit = .* must be finite and > 0", a=np.zeros(4), t=np.ones(3))
    refuse(ValueError, "ptr must start at 0", group_ptr=[0, 2, 3])
    refuse(ValueError, "an edge joins two groups", group_ptr=[0, 2, 4])
    refuse(ValueError, "block must be a positive integer", block=0)
    refuse(ValueError, "budget_bytes must be an integer", budget_bytes=0)
    if not torch.cuda.is_available():
        refuse(_lib.NativeLibraryError, "runs on the device")                  # the device comes last
    with pytest.raises(ValueError, match="member is"):
        bodies.label_reference(np.ones(3, dtype=bool), [], [])
    with pytest.raises(ValueError, match="outside 0 .. S - 1"):
        bodies.label_reference(np.ones((2, 2), dtype=bool), [0], [2])


def test_the_signature_is_declared_in_both_places():
    hdr = open(os.path.join(ROOT, "include", "geobipy_amd.h")).read()
    decl = re.search(r"gbp_status gbp_bodies_label\(([^;]*)\);", hdr)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["gbp_bodies_label"]
    assert res is _lib.c_int and len(args) == len(params) == 19
    for p, arg in zip(params, args):
        want = _lib.c_void_p if "*" in p else {"int": _lib.c_int, "double": _lib.ctypes.c_double}[p.split()[0]]
        assert arg is want, p
    from geobipy_amd import build
    assert "gbp_bodies.h" in build.HEADERS
    assert '#include "gbp_bodies.h"' in open(os.path.join(build.CSRC, "gbp_fdem.hip")).read()
