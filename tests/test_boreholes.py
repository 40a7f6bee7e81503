"""Borehole logs as evidence for sections, the host side (geobipy_amd.boreholes: Logs, load / save, attach, score_reference;
DESIGN.md 3.31): no GPU.  The rule is held to closed forms written out here, the attachment and the files to what they must give, and
the three planted lines of test_spatial_sections.py show what a log is for: alone the middle line sits on its decoy, with one log at
one sounding it sits on the true family."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, boreholes, ensembles, sections
from test_spatial_sections import DECOY, S_LINES, Z1_LINES, planted_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def one_sounding(models, K=4):
    """k [1, n], edges, sigma [1, n, K], rows [1, n], n_used [1] of ``models``: a list of (interfaces, conductivities)."""
    n = len(models)
    k = np.zeros((1, n), dtype=np.int32)
    edges, sigma = np.full((1, n, K), np.inf), np.full((1, n, K), np.nan)
    for m, (e, s) in enumerate(models):
        k[0, m] = len(s)
        edges[0, m, :len(e)] = e
        sigma[0, m, :len(s)] = s
    return k, edges, sigma, np.arange(n, dtype=np.int32)[None, :], np.array([n], dtype=np.int32)


def one_log(tops, bottoms, values=None, sds=None, cls=None, collar=np.nan):
    I = len(tops)
    return boreholes.Logs([0.0], [0.0], [collar], [0, I], tops, bottoms, values, sds, cls)


def at_sounding_0(var=0.0, shift=0.0, bores=(0,)):
    A = len(bores)
    return dict(att_ptr=np.array([0, A], dtype=np.int32), att_sounding=np.zeros(A, dtype=np.int32), att_bore=np.array(bores, dtype=np.int32),
                att_var=np.full(A, var), att_shift=np.full(A, shift), att_distance=np.zeros(A))


def rule(models, logs, **kw):
    att = kw.pop("att", None) or at_sounding_0(kw.pop("var", 0.0), kw.pop("shift", 0.0))
    return boreholes.score_reference(*one_sounding(models), att, logs, **kw)


# the models of the closed forms: a half-space, two layers with the interface at 10 m, three layers with interfaces at 10 and 30 m
HALF, TWO, THREE = ([], [0.1]), ([10.0], [0.01, 1.0]), ([10.0, 30.0], [0.01, 1.0, 0.1])
MODELS = [HALF, TWO, THREE]


# ---- the rule against closed forms --------------------------------------------------------------------------------------------------

def test_measured_intervals_against_closed_forms():
    gauss = lambda mean, value, sd, var=0.0: -((mean - value) ** 2) / (2.0 * (sd * sd + var))      # noqa: E731
    # inside one layer (2 .. 8 m): the mean is the layer's value
    got = rule(MODELS, one_log([2.0], [8.0], [-1.5], [0.2]))
    assert np.allclose(got["score"][0], [gauss(-1.0, -1.5, 0.2), gauss(-2.0, -1.5, 0.2), gauss(-2.0, -1.5, 0.2)], rtol=4 * U, atol=0)
    assert np.array_equal(got["score"][0], got["part"][0]) and got["skipped"].tolist() == [0]
    # straddling one interface (6 .. 16 m over the interface at 10 m): mean = (4 * -2 + 6 * 0) / 10 = -0.8
    got = rule(MODELS, one_log([6.0], [16.0], [-0.5], [0.1]))
    assert np.allclose(got["score"][0], [gauss(-1.0, -0.5, 0.1), gauss(-0.8, -0.5, 0.1), gauss(-0.8, -0.5, 0.1)], rtol=8 * U, atol=0)
    # an edge exactly on an interface (10 .. 20 m and 4 .. 10 m): no sliver of the neighbouring layer
    got = rule(MODELS, one_log([4.0, 10.0], [10.0, 20.0], [-2.0, 0.0], [0.1, 0.1]))
    assert got["score"][0, 1] == 0.0 and got["score"][0, 2] == 0.0 and got["score"][0, 0] == gauss(-1.0, -2.0, 0.1) + gauss(-1.0, 0.0, 0.1)
    # below the last interface (40 .. 50 m): the last layer, to any depth
    got = rule(MODELS, one_log([40.0], [50.0], [-1.0], [0.3]))
    assert got["score"][0].tolist() == [0.0, gauss(0.0, -1.0, 0.3), 0.0]
    # a gap (2 .. 8 m, then 20 .. 40 m over the interface at 30 m): what lies between says nothing
    got = rule(MODELS, one_log([2.0, 20.0], [8.0, 40.0], [-2.0, -0.5], [0.1, 0.1]))
    assert np.allclose(got["score"][0, 2], gauss(-2.0, -2.0, 0.1) + gauss(-0.5, -0.5, 0.1), rtol=0, atol=1e-28)
    assert np.allclose(got["score"][0, 1], gauss(0.0, -0.5, 0.1), rtol=4 * U, atol=0)
    # var = 0 against var > 0: the walk widens the Gaussian, nothing else
    tight, wide = rule(MODELS, one_log([2.0], [8.0], [-1.5], [0.2])), rule(MODELS, one_log([2.0], [8.0], [-1.5], [0.2]), var=0.05)
    assert np.allclose(wide["score"][0], tight["score"][0] * 0.04 / 0.09, rtol=8 * U, atol=0) and np.all(wide["score"] > tight["score"])


def test_shifts_ground_and_skipped_intervals():
    gauss = lambda mean, value, sd: -((mean - value) ** 2) / (2.0 * sd * sd)      # noqa: E731
    log = one_log([0.0, 4.0, 12.0], [4.0, 12.0, 20.0], [-1.0, -1.0, -1.0], [0.1, 0.1, 0.1], collar=100.0)
    # shift +2 (the sounding's ground lies 2 m above the collar): 2 .. 6, 6 .. 14, 14 .. 22 below the sounding
    got = rule([TWO], log, shift=2.0)
    want = gauss(-2.0, -1.0, 0.1) + gauss((4 * -2.0 + 4 * 0.0) / 8.0, -1.0, 0.1) + gauss(0.0, -1.0, 0.1)
    assert np.allclose(got["score"][0, 0], want, rtol=8 * U, atol=0) and got["skipped"].tolist() == [0]
    # shift -6: -6 .. -2 lies wholly above the ground (skipped, counted), -2 .. 6 is cut by it to 0 .. 6, then 6 .. 14
    got = rule([TWO], log, shift=-6.0)
    want = gauss(-2.0, -1.0, 0.1) + gauss((4 * -2.0 + 4 * 0.0) / 8.0, -1.0, 0.1)
    assert np.allclose(got["score"][0, 0], want, rtol=8 * U, atol=0) and got["skipped"].tolist() == [1]
    # shift -4: the first interval ends exactly at the ground: b' = 0 <= t' = 0, skipped
    assert rule([TWO], log, shift=-4.0)["skipped"].tolist() == [1]
    # everything above the ground: the score is 0.0 and all three are counted
    got = rule([TWO], log, shift=-25.0)
    assert got["score"][0, 0] == 0.0 and got["skipped"].tolist() == [3]
    # the cut interval's mean is taken over what is left of it (h = b' - t'), not over its logged length
    cut = rule([TWO], one_log([0.0], [16.0], [-1.0], [0.1], collar=0.0), shift=-4.0)      # 0 .. 12: (10 * -2 + 2 * 0) / 12
    assert np.allclose(cut["score"][0, 0], gauss(-20.0 / 12.0, -1.0, 0.1), rtol=8 * U, atol=0)


def test_lithology_intervals_against_closed_forms():
    classes = ([-2.0, 0.0], [0.2, 0.2])
    # a single class: P = 1 whatever the layer, the term is ln 1 = 0
    got = rule(MODELS, one_log([2.0, 8.0], [8.0, 40.0], cls=[0, 0]), classes=([-1.0], [0.3]))
    assert np.all(got["score"] == 0.0) and np.all(got["part"] == 0.0)
    # two far-apart classes: a layer at one mean has P = 1 for its own class (term 0) and ~0 for the other: the floor's limit
    got = rule([TWO], one_log([2.0, 12.0], [8.0, 20.0], cls=[0, 1]), classes=classes)
    assert abs(got["score"][0, 0]) <= 1e-15
    got = rule([TWO], one_log([2.0, 12.0], [8.0, 20.0], cls=[1, 0]), classes=classes, class_floor=1e-4)
    assert np.allclose(got["score"][0, 0], 2.0 * np.log(1e-4), rtol=1e-12, atol=0)
    # halfway between two equal classes P = 1 / 2; with priors 3 : 1 it is 3 / 4 and 1 / 4
    mid = [([], [0.1])]
    f = 1e-6
    got = rule(mid, one_log([0.0], [5.0], cls=[0]), classes=classes)
    assert np.allclose(got["score"][0, 0], np.log(f + (1 - f) * 0.5), rtol=0, atol=4 * U)
    for c, share in ((0, 0.75), (1, 0.25)):
        got = rule(mid, one_log([0.0], [5.0], cls=[c]), classes=classes + ([3.0, 1.0],))
        assert np.allclose(got["score"][0, 0], np.log(f + (1 - f) * share), rtol=0, atol=8 * U)
        again = rule(mid, one_log([0.0], [5.0], cls=[c]), classes=classes + ([0.75, 0.25],))        # only the ratios count
        assert np.allclose(again["score"][0, 0], got["score"][0, 0], rtol=0, atol=64 * U)      # (a few roundings of l, about 3 in size)
    # a straddling interval: the mean of P over the segments, written out (4 m at P0(-2) and 6 m at P0(0))
    cl = ([-2.0, 0.0], [0.5, 1.0])

    def posterior0(a, var):
        l = [-0.5 * np.log(s * s + var) - (a - m) ** 2 / (2 * (s * s + var)) for m, s in zip(*cl)]
        return 1.0 / (1.0 + np.exp(l[1] - l[0]))

    for var in (0.0, 0.3):
        got = rule([TWO], one_log([6.0], [16.0], cls=[0]), classes=cl, var=var)
        want = np.log(f + (1 - f) * (4.0 * posterior0(-2.0, var) + 6.0 * posterior0(0.0, var)) / 10.0)
        assert np.allclose(got["score"][0, 0], want, rtol=0, atol=16 * U)
    assert posterior0(-2.0, 0.3) < posterior0(-2.0, 0.0)                       # the walk blurs the classes


def test_zeros_orders_and_dtypes():
    k, edges, sigma, rows, n_used = one_sounding(MODELS + [THREE])
    k = np.concatenate([k, k]); edges = np.concatenate([edges, edges]); sigma = np.concatenate([sigma, sigma])      # noqa: E702
    rows = np.array([[0, 1, 2, 3], [2, -1, 7, 3]], dtype=np.int32)
    k[1, 3] = 0                                                                # an empty slot
    logs = boreholes.Logs([0.0, 5.0], [0.0, 0.0], None, [0, 2, 3], [2.0, 8.0, 5.0], [8.0, 40.0, 25.0], [-1.0, -1.0, np.nan], [0.2, 0.2, np.nan], [-1, -1, 1])
    att = dict(att_ptr=np.array([0, 2, 3]), att_sounding=np.array([0, 0, 1]), att_bore=np.array([0, 1, 0]), att_var=np.array([0.0, 0.01, 0.02]),
               att_shift=np.zeros(3), att_distance=np.array([0.0, 1.0, 2.0]))
    cl = ([-2.0, -1.0, 0.0], [0.3, 0.3, 0.3])
    got = boreholes.score_reference(k, edges, sigma, rows, np.array([3, 4]), att, logs, classes=cl, terms=True)
    assert got["score"].dtype == np.float64 and got["skipped"].dtype == np.int32 and got["part"].shape == (3, 4)
    assert got["score"][0, 3] == 0.0 and got["part"][0, 3] == 0.0              # m >= n_used
    assert got["score"][1, 1] == 0.0 and got["score"][1, 2] == 0.0 and got["score"][1, 3] == 0.0      # row -1, row past the slots, k = 0
    assert np.array_equal(got["score"][0], (np.zeros(4) + got["part"][0]) + got["part"][1]) and np.array_equal(got["score"][1], got["part"][2])
    assert got["score"][0, 2] != 0.0 and got["score"][1, 0] == got["part"][2, 0] != 0.0
    assert np.array_equal(got["terms"][0].sum(axis=0), got["part"][0]) and got["terms"][1].shape == (1, 4)
    ld = boreholes.score_reference(k, edges, sigma, rows, np.array([3, 4]), att, logs, classes=cl, dtype=np.longdouble)
    assert ld["score"].dtype == np.longdouble and np.allclose(ld["score"].astype(np.float64), got["score"], rtol=1e-13, atol=1e-13)
    none = dict(att, att_ptr=np.array([0, 0, 0]), att_sounding=np.zeros(0, int), att_bore=np.zeros(0, int), att_var=np.zeros(0), att_shift=np.zeros(0))
    assert np.all(boreholes.score_reference(k, edges, sigma, rows, np.array([3, 4]), none, logs, classes=cl)["score"] == 0.0)


# ---- attachment ---------------------------------------------------------------------------------------------------------------------

def test_attach_takes_the_nearest_sounding_of_every_line():
    x = np.array([0.0, 10.0, 20.0, 30.0, 5.0, 15.0, 25.0, 0.0, 10.0, 20.0])
    y = np.array([0.0, 0.0, 0.0, 0.0, 100.0, 100.0, 100.0, 1000.0, 1000.0, 1000.0])
    ptr, n_used = [0, 4, 7, 10], np.array([3, 3, 0, 3, 3, 3, 3, 3, 3, 3])
    logs = boreholes.Logs([21.0, 10.0], [0.0, 50.0], [50.0, 60.0], [0, 1, 2], [0.0, 0.0], [5.0, 5.0], [-1.0, -1.0], [0.1, 0.1])
    att = boreholes.attach(x, y, logs, ptr, n_used, max_distance=80.0)
    # borehole 0 (21, 0): sounding 2 is nearest but has no models -> 1 and 3 tie at 9 / 11? no: 3 is at 9 m, 1 at 11 m -> 3; line B is 100 m off
    # borehole 1 (10, 50): line A sounding 1 at 50 m; line B soundings 4 and 5 tie at hypot(5, 50) -> the lower index, 4
    assert list(zip(att["att_sounding"].tolist(), att["att_bore"].tolist())) == [(1, 1), (3, 0), (4, 1)]
    assert att["att_ptr"].tolist() == [0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 3] and att["att_ptr"].dtype == np.int32
    assert att["att_distance"].tolist() == [50.0, 9.0, float(np.hypot(5.0, 50.0))]
    assert np.array_equal(att["att_var"], 0.1 * 0.1 * att["att_distance"] / 100.0) and np.all(att["att_shift"] == 0.0)
    assert boreholes.attach(x, y, logs, ptr, None, max_distance=80.0)["att_sounding"].tolist() == [1, 2, 4]       # every sounding has models
    assert boreholes.attach(x, y, logs, ptr, n_used, max_distance=9.0)["att_sounding"].tolist() == [3]            # <= : at the distance itself
    assert boreholes.attach(x, y, logs, ptr, n_used, max_distance=8.9)["att_sounding"].size == 0
    far = boreholes.attach(x, y, logs, ptr, n_used, max_distance=2000.0, tau=0.2, length=50.0)                    # all three lines, both logs
    assert far["att_sounding"].size == 6 and np.array_equal(far["att_var"], 0.2 * 0.2 * far["att_distance"] / 50.0)
    assert np.all(np.diff(far["att_sounding"].astype(np.int64) * 2 + far["att_bore"]) > 0)                        # sorted by s, then b
    on = boreholes.attach(x, y, boreholes.Logs([30.0], [0.0], None, [0, 0], [], []), ptr, n_used, max_distance=1.0)
    assert on["att_distance"].tolist() == [0.0] and on["att_var"].tolist() == [0.0]                               # d = 0 gives 0
    surface = 40.0 + np.arange(10.0)
    assert boreholes.attach(x, y, logs, ptr, n_used, max_distance=80.0, surface=surface)["att_shift"].tolist() == [41.0 - 60.0, 43.0 - 50.0, 44.0 - 60.0]
    nan_collar = boreholes.Logs([21.0], [0.0], [np.nan], [0, 0], [], [])
    assert boreholes.attach(x, y, nan_collar, ptr, n_used, max_distance=80.0)["att_shift"].tolist() == [0.0]
    with pytest.raises(ValueError, match="collar"):
        boreholes.attach(x, y, nan_collar, ptr, n_used, max_distance=80.0, surface=surface)
    with pytest.raises(TypeError):
        boreholes.attach(x, y, logs, ptr, n_used)                               # max_distance is not guessed
    for kw, match in ((dict(max_distance=0.0), "max_distance"), (dict(max_distance=80.0, tau=0.0), "tau"), (dict(max_distance=80.0, length=np.inf), "length"),
                      (dict(max_distance=80.0, surface=surface[:3]), "surface")):
        with pytest.raises(ValueError, match=match):
            boreholes.attach(x, y, logs, ptr, n_used, **kw)
    with pytest.raises(ValueError, match="n_used"):
        boreholes.attach(x, y, logs, ptr, n_used[:4], max_distance=80.0)
    with pytest.raises(ValueError, match="ptr"):
        boreholes.attach(x, y, logs, [0, 4], n_used, max_distance=80.0)
    with pytest.raises(ValueError, match="Logs"):
        boreholes.attach(x, y, "logs.npz", ptr, n_used, max_distance=80.0)


# ---- files --------------------------------------------------------------------------------------------------------------------------

def some_logs():
    return boreholes.Logs([1.5, -2.25, 1e6 / 3.0], [0.0, 7.0, 0.1], [101.3, np.nan, 0.0], [0, 2, 3, 6], [0.0, 2.0, 1.0, 0.0, 0.7, 5.5], [2.0, 3.5, 4.0, 0.7, 1.1, 6.0],
                          [-1.2, np.nan, -0.3, np.nan, 1.0 / 3.0, np.nan], [0.1, np.nan, 0.25, np.nan, 0.05, np.nan], [-1, 2, -1, 0, -1, 15], ["A", "B-2", "c 3"])


@pytest.mark.parametrize("suffix", [".npz", ".csv"])
def test_load_and_save_round_trip(tmp_path, suffix):
    logs = some_logs()
    path = boreholes.save(logs, str(tmp_path / ("logs" + suffix)))
    back = boreholes.load(path)
    for name, a in logs.arrays().items():
        b = back.arrays()[name]
        assert a.dtype == b.dtype or name == "name", name
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name      # every bit of every number
    assert back.name == logs.name and back.n_boreholes == 3 and back.n_intervals == 6
    assert boreholes.load(back) is back


def test_the_text_table_by_hand(tmp_path):
    path = tmp_path / "hand.txt"
    path.write_text("# two boreholes\nname,x,y,collar,top,bottom,value,sd,class\nP1,10,20,,0,2,-1.5,0.1,\nP1,10,20,nan,2,4,,,1\n\nP2,0,0,55.5,1,3,-2,0.2,-1\n")
    logs = boreholes.load(str(path))
    assert logs.name == ["P1", "P2"] and logs.ptr.tolist() == [0, 2, 3] and logs.cls.tolist() == [-1, 1, -1]
    assert np.isnan(logs.collar[0]) and logs.collar[1] == 55.5 and np.isnan(logs.value[1]) and logs.sd.tolist()[::2] == [0.1, 0.2]
    for text, match in (("x,y\n", "header"), ("name,x,y,collar,top,bottom,value,sd,class\nP1,1,2,3\n", "fields"),
                        ("name,x,y,collar,top,bottom,value,sd,class\nP1,a,0,,0,1,-1,0.1,\n", "not a number"),
                        ("name,x,y,collar,top,bottom,value,sd,class\n,0,0,,0,1,-1,0.1,\n", "name is empty"),
                        ("name,x,y,collar,top,bottom,value,sd,class\nP1,0,0,,0,1,-1,0.1,\nP2,0,0,,0,1,-1,0.1,\nP1,0,0,,1,2,-1,0.1,\n", "follow each other"),
                        ("name,x,y,collar,top,bottom,value,sd,class\nP1,0,0,,0,1,-1,0.1,\nP1,1,0,,1,2,-1,0.1,\n", "changes its x, y or collar"),
                        ("name,x,y,collar,top,bottom,value,sd,class\nP1,0,0,,0,1,-1,0.1,0.5\n", "integer"),
                        ("name,x,y,collar,top,bottom,value,sd,class\nP1,0,0,,1,2,-1,0.1,\nP1,0,0,,0,1,-1,0.1,\n", "ascend")):
        path.write_text(text)
        with pytest.raises(ValueError, match=match):
            boreholes.load(str(path))
    with pytest.raises(ValueError, match="without intervals"):
        boreholes.save(boreholes.Logs([0.0], [0.0], None, [0, 0], [], []), str(tmp_path / "empty.csv"))
    with pytest.raises(ValueError, match="names"):
        boreholes.save(boreholes.Logs([0.0, 1.0], [0.0, 0.0], None, [0, 1, 2], [0, 0], [1, 1], [0, 0], [1, 1], name=["a", "a"]), str(tmp_path / "twice.csv"))
    np.savez(str(tmp_path / "short.npz"), x=[0.0], y=[0.0])
    with pytest.raises(ValueError, match="holds no ptr, top, bottom"):
        boreholes.load(str(tmp_path / "short.npz"))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_logs_refuse_by_name():
    ok = dict(x=[0.0, 1.0], y=[0.0, 0.0], collar=[1.0, np.nan], ptr=[0, 2, 3], top=[0.0, 2.0, 0.0], bottom=[2.0, 3.0, 1.0], value=[-1.0, np.nan, -1.0],
              sd=[0.1, np.nan, 0.1], cls=[-1, 0, -1])
    boreholes.Logs(**ok)
    for change, match in ((dict(y=[0.0]), "one entry per borehole"), (dict(x=[0.0, np.inf]), "x and y must be finite"), (dict(collar=[1.0, np.inf]), "collar"),
                          (dict(ptr=[0, 2]), "Nb \\+ 1"), (dict(ptr=[0, 2, 4]), "start at 0, end at"), (dict(ptr=[1, 2, 3]), "start at 0"),
                          (dict(ptr=[0, 3, 2]), "start at 0, end at"), (dict(bottom=[2.0, 3.0]), "one entry per interval"),
                          (dict(top=[0.0, np.nan, 0.0]), "top and bottom must be finite"), (dict(top=[-1.0, 2.0, 0.0]), "0 <= top < bottom"),
                          (dict(bottom=[2.0, 2.0, 1.0]), "0 <= top < bottom"), (dict(top=[0.0, 1.5, 0.0]), "ascend and must not overlap"),
                          (dict(cls=[-1, -2, -1]), "-1 \\(measured\\)"), (dict(cls=[-1.0, 0.0, -1.0]), "integers"),
                          (dict(sd=[0.0, np.nan, 0.1]), "finite sd > 0"), (dict(value=[np.nan, np.nan, -1.0]), "finite value"),
                          (dict(value=[-1.0, -1.0, -1.0]), "exactly one kind"), (dict(name=["a"]), "name")):
        with pytest.raises(ValueError, match=match):
            boreholes.Logs(**dict(ok, **change))


def test_refusals_come_before_the_library():
    k, edges, sigma, rows, n_used = one_sounding(MODELS)
    lith, att = one_log([0.0], [5.0], cls=[2]), at_sounding_0()
    ref = lambda **kw: boreholes.score_reference(k, edges, sigma, rows, n_used, kw.pop("att", att), kw.pop("logs", lith), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="need classes"):
        ref()
    with pytest.raises(ValueError, match="name class 2, classes holds 2"):
        ref(classes=([0.0, 1.0], [1.0, 1.0]))
    for classes, match in ((([0.0], [1.0, 1.0]), "as many scales"), (([0.0, 1.0, 2.0], [1.0, 0.0, 1.0]), "positive"), (([0.0] * 17, [1.0] * 17), "1 to 16"),
                           (([0.0, 1.0, 2.0], [1.0, 1.0, 1.0], [1.0, 0.0, 1.0]), "priors"), (([0.0, 1.0, 2.0], [1.0, 1.0, 1.0], [1.0, 1.0]), "priors"),
                           (([0.0, 1.0, 2.0],), "means, scales")):
        with pytest.raises(ValueError, match=match):
            ref(classes=classes)
    for floor in (0.0, 1.0, -1e-3, True):
        with pytest.raises(ValueError, match="class_floor"):
            ref(classes=([0.0, 1.0, 2.0], [1.0, 1.0, 1.0]), class_floor=floor)
    for change, match in ((dict(att_ptr=np.array([0, 1, 1])), "S \\+ 1"), (dict(att_ptr=np.array([0, 2])), "end at the number of attachments"),
                          (dict(att_bore=np.array([1])), "0 .. Nb - 1"), (dict(att_var=np.array([-1.0])), "att_var"), (dict(att_shift=np.array([np.nan])), "att_shift"),
                          (dict(att_sounding=np.array([1])), "att_sounding"), (dict(att_var=np.zeros(2)), "one entry per attachment")):
        with pytest.raises(ValueError, match=match):
            ref(att=dict(att, **change), classes=([0.0, 1.0, 2.0], [1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="boreholes.attach returns"):
        ref(att=dict(att_ptr=[0, 1]))
    with pytest.raises(ValueError, match="Logs"):
        ref(logs="logs.csv")

    # the device entry: host tensors are refused after the shapes and values, and nothing loads the library
    tk, te, ts = torch.as_tensor(k), torch.as_tensor(edges), torch.as_tensor(sigma)
    ens = ensembles.Ensemble(tk, te, ts, torch.zeros(tk.shape, dtype=torch.float64), (tk > 0).sum(dim=1), 1, torch.zeros(1, dtype=torch.float64))
    trows, tnu = torch.as_tensor(rows), torch.as_tensor(n_used)
    meas = one_log([0.0], [5.0], [-1.0], [0.1])
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        boreholes.score(ens, trows, tnu, att, meas)
    with pytest.raises(_lib.NativeLibraryError, match="torch tensors"):
        boreholes.score(ens, rows, tnu, att, meas)
    with pytest.raises(ValueError, match="n_used is int32"):
        boreholes.score(ens, trows, tnu.long(), att, meas)
    with pytest.raises(ValueError, match="need classes"):
        boreholes.score(ens, trows, tnu, att, lith)
    with pytest.raises(ValueError, match="block"):
        boreholes.score(ens, trows, tnu, att, meas, block=0)
    with pytest.raises(ValueError, match="rows \\[S, n\\] with 1 <= n <= 1024"):
        boreholes.score(ens, torch.zeros((1, 1025), dtype=torch.int32), tnu, att, meas)
    with pytest.raises(ValueError, match="part \\[A, n\\]"):
        boreholes.log_predictive(torch.zeros((1, 3)), torch.zeros((1, 4)), tnu, att)

    # the keyword of sections: refused before any device work
    x, y = np.array([0.0]), np.array([0.0])
    for options, match in ((dict(logs=meas), "logs and max_distance"), (dict(logs=meas, max_distance=10.0, reach=3), "logs and max_distance"),
                           (dict(logs=meas, max_distance=0.0), "max_distance"), (dict(logs=lith, max_distance=10.0), "need classes"),
                           (dict(logs=meas, max_distance=10.0, class_floor=2.0), "class_floor"), ([meas], "dictionary")):
        with pytest.raises(ValueError, match=match):
            sections.sections(ens, x, y, 50.0, boreholes=options)
        with pytest.raises(ValueError, match=match):
            sections.spatial(ens, x, y, 50.0, max_distance=10.0, boreholes=options)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.sections(ens, x, y, 50.0, boreholes=dict(logs=meas, max_distance=10.0))


def test_the_command_line_takes_boreholes(capsys):
    path, kw = sections.parse_args(["run.npz", "--depth", "150", "--boreholes", "logs.csv", "--borehole-distance", "75"])
    assert kw["boreholes"] == dict(logs="logs.csv", max_distance=75.0, classes=None, class_floor=1e-6)
    _, kw = sections.parse_args(["run.npz", "--depth", "150", "--spatial", "300", "--spatial-draws", "8", "--boreholes", "logs.npz", "--borehole-distance", "75",
                                 "--class-means", "-2", "-0.5", "--class-scales", "0.2", "0.3", "--class-floor", "1e-3"])
    assert kw["boreholes"] == dict(logs="logs.npz", max_distance=75.0, classes=((-2.0, -0.5), (0.2, 0.3)), class_floor=1e-3) and kw["max_distance"] == 300.0
    assert "boreholes" not in sections.parse_args(["run.npz", "--depth", "150"])[1]
    base = ["run.npz", "--depth", "10"]
    for argv in (["--borehole-distance", "5"], ["--class-means", "1", "--class-scales", "1"], ["--class-floor", "0.1"], ["--boreholes", "l.csv"],
                 ["--boreholes", "l.csv", "--borehole-distance", "0"], ["--boreholes", "l.csv", "--borehole-distance", "5", "--class-means", "1"],
                 ["--boreholes", "l.csv", "--borehole-distance", "5", "--class-means", "1", "2", "--class-scales", "1"],
                 ["--boreholes", "l.csv", "--borehole-distance", "5", "--class-floor", "1"]):
        with pytest.raises(SystemExit):
            sections.parse_args(base + argv)
    capsys.readouterr()


def test_the_signature_declares_the_entry():
    res, args = _lib.SIGNATURES["gbp_borehole_score"]
    assert res is _lib.c_int and len(args) == 31 and args[-5] is _lib.ctypes.c_double and args[23:26] == [_lib.c_double_p] * 3
    with open(os.path.join(ROOT, "include", "geobipy_amd.h")) as f:
        hdr = f.read()
    assert "gbp_status gbp_borehole_score(" in hdr
    decl = hdr[hdr.index("gbp_status gbp_borehole_score("):]
    assert decl[:decl.index(";")].count(",") == 30                            # 31 parameters
    from geobipy_amd import build
    assert "gbp_boreholes.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "gbp_boreholes.h"))
    with open(os.path.join(build.CSRC, "gbp_fdem.hip")) as f:
        assert '#include "gbp_boreholes.h"' in f.read()


# ---- the planted lines --------------------------------------------------------------------------------------------------------------

BORE_ROW = S_LINES + 3          # the 4th sounding of the middle line
LITH_CLASSES = ([-2.0, -0.5, -1.5], [0.2, 0.2, 0.2])


def planted_log(kind, truth):
    """One borehole at sounding ``BORE_ROW`` of the planted lines with a 2 m log from 0 to 100 m that follows the true layering (-2.0
    above the first interface at truth[row], -0.5 down to 80 m, -1.5 below; an interval takes the layer of its centre): ``kind``
    "induction" (sd 0.1 decade) or "lithology" (classes 0, 1, 2 of LITH_CLASSES)."""
    x, y = 25.0 * 3, 100.0
    top = np.arange(0.0, 100.0, 2.0)
    mid = top + 1.0
    layer = np.where(mid < truth[BORE_ROW], 0, np.where(mid < 80.0, 1, 2))
    if kind == "induction":
        return boreholes.Logs([x], [y], None, [0, top.size], top, top + 2.0, np.array([-2.0, -0.5, -1.5])[layer], np.full(top.size, 0.1))
    return boreholes.Logs([x], [y], None, [0, top.size], top, top + 2.0, None, None, layer)


def test_one_log_decides_the_planted_middle_line():
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    S, n = k.shape
    rows, n_used = np.tile(np.arange(n, dtype=np.int32), (S, 1)), np.full(S, n)
    middle = np.arange(S_LINES, 2 * S_LINES)
    partner = sections.partners(ptr, n_used)
    d2 = sections.cross_distance_reference(k, edges, sigma, rows, partner, 0.0, Z1_LINES)
    g = sections.steps(x, y, ptr=ptr)
    alone = sections.track_reference(ptr, None, g, d2, n_used)
    share = alone["marginal"][middle, :10].sum(axis=1)
    assert np.all(alone["state"][middle] < 10) and np.all(share > 0.625)
    for kind in ("induction", "lithology"):
        logs = planted_log(kind, truth)
        att = boreholes.attach(x, y, logs, ptr, n_used, max_distance=1.0)
        assert att["att_sounding"].tolist() == [BORE_ROW] and att["att_distance"].tolist() == [0.0]      # that sounding only: the others are >= 25 m away
        res = boreholes.score_reference(k, edges, sigma, rows, n_used, att, logs, classes=LITH_CLASSES if kind == "lithology" else None)
        sc = res["score"]
        assert np.all(sc[np.arange(S) != BORE_ROW] == 0.0) and res["skipped"].tolist() == [0]
        print("%s log at row %d: decoy models at most %.2f, true family %.2f .. %.2f" % (kind, BORE_ROW, sc[BORE_ROW, :10].max(), sc[BORE_ROW, 10:].min(),
                                                                                         sc[BORE_ROW, 10:].max()))
        assert sc[BORE_ROW, :10].max() < sc[BORE_ROW, 10:].min() - 50.0
        with_log = sections.track_reference(ptr, sc, g, d2, n_used)
        share = with_log["marginal"][middle, :10].sum(axis=1)
        print("    middle line", with_log["state"][middle], "decoy share at most %.3g" % share.max())
        assert np.all(with_log["state"][middle] >= 10) and np.all(share < 1e-3)
        assert np.all(np.abs(edges[middle, with_log["state"][middle], 0] - truth[middle]) <= 4.0)
        outer = np.concatenate([np.arange(S_LINES), np.arange(2 * S_LINES, S)])
        assert np.array_equal(with_log["state"][outer], alone["state"][outer])      # the line is solved alone: the outer lines keep their paths
    assert np.all(np.abs(edges[middle, alone["state"][middle], 0] - DECOY) <= 2.0)
