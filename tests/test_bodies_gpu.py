"""Connected bodies on the device (csrc/gbp_bodies.h k_bodies_label through gbp_bodies_label; geobipy_amd.bodies label / summary /
connected / reach; sections.draw_bodies, sections(bodies=), spatial(bodies=)), held to ``bodies.label_reference``.

The outputs are integers and canonical -- the label of a body is its smallest linear index -- so the device is compared to the rule with
``==`` in every cell of every realisation: label, cells and measure_q, nothing left out.  The shapes are the smallest at which the kernel
can go wrong: columns around the 64-cell chunk (1, 2, 63, 64, 65, 130: the carry of a run across chunks), more soundings than the
workgroup has waves (70 > 16), realisations around a wave's width, member densities below, near and above the lattice's percolation
point (0.59: long tortuous bodies), graphs with branching, loops, isolated soundings and an empty group, and the serpentine."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, bodies, sections
from test_bodies import line_edges, serpentine
from test_families_gpu import _to_device
from test_spatial_sections import S_LINES, SPACING, Z1_LINES, lattice_graph, planted_lines, star_graph


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else v) for n, v in d.items()}


def three_lines(cross=True):
    """Three lines of five soundings; with ``cross`` every second sounding is tied to the line beside it."""
    eu = [l * 5 + s for l in range(3) for s in range(4)]
    ev = [u + 1 for u in eu]
    if cross:
        eu += [0, 2, 4, 7, 9]
        ev += [5, 7, 9, 12, 14]
    return np.array(eu), np.array(ev), 15


def ragged_graph():
    """A line of three, an isolated sounding, an empty group, and a triangle listed backwards and twice."""
    return np.array([0, 2, 6, 5, 6, 4, 6]), np.array([1, 1, 4, 4, 5, 6, 5]), 7, np.array([0, 3, 4, 4, 7])


GRAPHS = {"lattice": lambda: lattice_graph() + (None,), "star": lambda: (star_graph()[0], star_graph()[1], 5, None),
          "three_lines": lambda: three_lines() + (None,), "three_alone": lambda: three_lines(False) + (None,), "ragged": ragged_graph}

# (graph or "line", S, C, R, density, with a / t)
CASES = [("line", 1, 1, 1, 0.59, True), ("line", 2, 2, 3, 0.59, False), ("line", 7, 63, 65, 0.59, True), ("line", 70, 64, 3, 0.3, False),
         ("line", 70, 65, 3, 0.3, True), ("line", 70, 65, 3, 0.59, True), ("line", 70, 65, 3, 0.9, False), ("line", 70, 130, 1, 0.59, True),
         ("line", 2, 130, 65, 0.9, True), ("line", 70, 1, 3, 0.59, False), ("line", 1, 65, 3, 0.59, True), ("line", 7, 2, 1, 0.3, True),
         ("lattice", 12, 65, 3, 0.59, True), ("lattice", 12, 2, 65, 0.59, False), ("star", 5, 64, 3, 0.59, True), ("star", 5, 130, 1, 0.3, False),
         ("three_lines", 15, 63, 3, 0.59, True), ("three_lines", 15, 65, 3, 0.9, False), ("three_alone", 15, 65, 3, 0.59, True),
         ("ragged", 7, 65, 3, 0.59, True), ("ragged", 7, 1, 65, 0.59, False), ("ragged", 7, 130, 3, 0.9, True)]


@functools.lru_cache(maxsize=None)
def _case(name, S, C, R, density, measure):
    """(raster [R, S, C], lo, hi, eu, ev, group_ptr, a, t, the rule's result): computed once."""
    rng = np.random.default_rng(1000 * S + 10 * C + R + int(100 * density))
    if name == "line":
        eu, ev = line_edges(S)
        group_ptr = None
    else:
        eu, ev, S_, group_ptr = GRAPHS[name]()
        assert S_ == S
    raster = rng.random((R, S, C))
    raster[rng.random((R, S, C)) < 0.02] = np.nan                              # never a member
    lo, hi = 0.25, 0.25 + density                                              # two-sided: both compares decide
    a = rng.uniform(5.0, 60.0, S) if measure else None
    t = rng.uniform(0.5, 12.0, C) if measure else None
    ref = bodies.label_reference(bodies.member_reference(raster, lo, hi), eu, ev, a=a, t=t)
    return raster, lo, hi, eu, ev, group_ptr, a, t, ref


def _device(case, **kw):
    raster, lo, hi, eu, ev, group_ptr, a, t, _ = case
    out = bodies.label(torch.as_tensor(raster).to(_dev()), lo, hi, eu, ev, group_ptr=group_ptr, a=a, t=t, **kw)
    torch.cuda.synchronize()
    return out


def _equal_to_the_rule(got, ref, S, C):
    g = _numpy(got)
    assert g["label"].dtype == np.int32 and g["cells"].dtype == np.int32 and g["label"].shape == ref["label"].shape
    assert np.array_equal(g["label"], ref["label"])
    assert np.array_equal(g["cells"], ref["cells"])
    G = g["group_ptr"].size - 1
    assert g["sweeps"].dtype == np.int32 and g["sweeps"].shape == (ref["label"].shape[0], G)
    nodes = np.diff(g["group_ptr"]) * C
    assert np.all(g["sweeps"] >= 0) and np.all(g["sweeps"] <= np.maximum(nodes, 0)[None, :])
    if "measure_q" in ref:
        assert g["measure_q"].dtype == np.int64 and np.array_equal(g["measure_q"], ref["measure_q"])
        assert g["unit"] == ref["unit"] and np.array_equal(g["measure"], ref["measure"])
    else:
        assert "measure_q" not in g and "measure" not in g
    return g


@pytest.mark.parametrize("name,S,C,R,density,measure", CASES)
def test_the_device_against_the_rule(name, S, C, R, density, measure):
    case = _case(name, S, C, R, density, measure)
    g = _equal_to_the_rule(_device(case), case[8], S, C)
    print("%s S=%d C=%d R=%d density %.2f: %d groups, %d bodies, the largest of %d cells, at most %d sweeps"
          % (name, S, C, R, density, g["group_ptr"].size - 1, int((g["cells"] > 0).sum()), int(g["cells"].max(initial=0)), int(g["sweeps"].max(initial=0))))


def test_default_groups_are_the_lines_and_explicit_groups_change_nothing():
    case = _case("three_alone", 15, 65, 3, 0.59, True)
    lines = _device(case)
    assert np.array_equal(lines["group_ptr"], [0, 5, 10, 15])
    one = _device(case[:5] + (np.array([0, 15]),) + case[6:])
    two = _device(case[:5] + (np.array([0, 0, 10, 15, 15]),) + case[6:])       # empty groups at both ends
    for name in ("label", "cells", "measure_q"):
        assert torch.equal(one[name], lines[name]) and torch.equal(two[name], lines[name]), name
    assert np.array_equal(_device(_case("three_lines", 15, 63, 3, 0.59, True))["group_ptr"], [0, 15])
    assert np.array_equal(_device(_case("ragged", 7, 65, 3, 0.59, True))["group_ptr"], [0, 3, 4, 4, 7])
    assert bool((two["sweeps"][:, [0, 3]] == 0).all())


def test_the_serpentine_is_one_body():
    S, C = 70, 65
    member = serpentine(S, C)
    raster = np.where(member, 1.0, np.nan)[None]
    eu, ev = line_edges(S)
    a, t = np.linspace(1.0, 2.0, S), np.linspace(3.0, 1.0, C)
    ref = bodies.label_reference(member[None], eu, ev, a=a, t=t)
    assert ref["cells"][0, 0, 0] == 35 * C + 35 == member.sum() and np.all(ref["label"][0][member] == 0)
    for lo, hi in ((1.0, 1.0), (-np.inf, np.inf), (0.5, np.inf)):              # lo == hi, and the one-sided thresholds
        got = bodies.label(torch.as_tensor(raster).to(_dev()), lo, hi, eu, ev, a=a, t=t)
        g = _equal_to_the_rule(got, ref, S, C)
        assert g["sweeps"].shape == (1, 1) and 1 <= g["sweeps"][0, 0] <= S * C
    print("the serpentine of %d cells took %d sweeps" % (member.sum(), g["sweeps"][0, 0]))


def test_a_call_repeats_its_bits_and_the_cut_changes_nothing():
    case = _case("line", 7, 63, 65, 0.59, True)
    first, again, cut = _device(case), _device(case), _device(case, block=1)
    few = _device(case, budget_bytes=16 * 7 * 63 * 9)                          # blocks of nine realisations
    raster = case[0]
    one = _device((raster[:1],) + case[1:])
    for name in ("label", "cells", "measure_q", "measure", "sweeps"):
        assert torch.equal(again[name], first[name]) and torch.equal(cut[name], first[name]) and torch.equal(few[name], first[name]), name
        assert torch.equal(one[name][0], first[name][0]), name
    assert one["unit"] == first["unit"]


def test_the_c_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    R, S, C, E, G = 2, 4, 3, 3, 2
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    a = dict(R=R, S=S, C=C, E=E, G=G, gp=torch.tensor([0, 2, 4], dtype=torch.int64, device=dev), eu=i32([0, 1, 2]), ev=i32([1, 0, 3]),
             v=torch.ones((R, S, C), dtype=torch.float64, device=dev), lo=0.5, hi=1.5, a=torch.ones(S, dtype=torch.float64, device=dev),
             t=torch.ones(C, dtype=torch.float64, device=dev), unit=2.0 ** -30, label=torch.full((R, S, C), 7, dtype=torch.int32, device=dev),
             cells=torch.full((R, S, C), 7, dtype=torch.int32, device=dev), mq=torch.full((R, S, C), 7, dtype=torch.int64, device=dev),
             sweeps=torch.full((R, G), 7, dtype=torch.int32, device=dev))
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                    # noqa: E731

    def call(**kw):
        b = dict(a, **kw)
        return lib.gbp_bodies_label(*[p(b[name]) for name in ("R", "S", "C", "E", "G", "gp", "eu", "ev", "v", "lo", "hi", "a", "t", "unit", "label", "cells",
                                                            "mq", "sweeps")], st)

    gp = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)              # noqa: E731
    for kw in (dict(R=0), dict(R=65537), dict(S=-1), dict(C=0), dict(C=4097), dict(E=-1), dict(E=2 ** 30), dict(G=-1), dict(G=5), dict(G=0),
               dict(R=65536, S=2 ** 15, C=1), dict(a=None), dict(t=None), dict(unit=0.0), dict(unit=float("inf")), dict(unit=float("nan")),
               dict(gp=None), dict(v=None), dict(label=None), dict(cells=None), dict(sweeps=None), dict(mq=None), dict(eu=None), dict(ev=None),
               dict(gp=gp([1, 2, 4])), dict(gp=gp([0, 2, 3])), dict(gp=gp([0, 5, 4])), dict(ev=i32([1, 0, 4])), dict(eu=i32([-1, 1, 2])),
               dict(eu=i32([2, 1, 0]), ev=i32([3, 0, 1])), dict(ev=i32([1, 2, 3])), dict(eu=i32([0, 2, 2]), ev=i32([1, 1, 3]))):
        assert call(**kw) != 0 and b"gbp_bodies_label" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((a[name] == 7).all()) for name in ("label", "cells", "mq", "sweeps"))      # nothing was written
    assert call(S=0, E=0, G=0, gp=None, v=None) == 0                           # no sounding: OK without a launch
    torch.cuda.synchronize()
    assert bool((a["label"] == 7).all())
    assert call(a=None, t=None, mq=None) == 0                                  # without a measure measure_q is not written
    torch.cuda.synchronize()
    assert bool((a["mq"] == 7).all()) and bool((a["label"] == torch.tensor([0, 0, 0, 0, 0, 0, 6, 6, 6, 6, 6, 6], device=dev).reshape(4, 3)).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert a["cells"][0].reshape(-1).tolist() == [6, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0] and a["mq"][1].reshape(-1)[[0, 6]].tolist() == [6 * 2 ** 30] * 2
    assert bool(((a["sweeps"] >= 1) & (a["sweeps"] <= 6)).all())


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

U = 2.0 ** -52
NEW = {"body_count", "body_largest_measure", "body_member_measure", "body_largest_share"}


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


@functools.lru_cache(maxsize=None)
def _planted():
    """The planted lines of test_spatial_sections.py with every interface rounded to a whole metre, so that a raster of 1 m cells holds
    the layers exactly: (ens on the device, k, edges, sigma, x, y, ptr)."""
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    edges = np.where(np.isfinite(edges), np.round(edges), edges)
    return _to_device(k, edges, sigma), k, edges, sigma, x, y, ptr


def test_the_bodies_of_the_planted_lines_alone():
    ens, k, edges, sigma, x, y, ptr = _planted()
    S, n = k.shape
    R, C = 64, int(Z1_LINES)
    depth_edges = np.arange(0.0, Z1_LINES + 1.0, 1.0)
    kw = dict(ptr=ptr, max_models=n, draws=R, seed=2)
    plain = sections.sections(ens, x, y, Z1_LINES, **kw)
    out = sections.sections(ens, x, y, Z1_LINES, bodies=dict(depth_edges=depth_edges, lo=0.1, log10=False), **kw)
    assert set(out) == set(plain) | NEW and not NEW & set(plain)
    for name in plain:                                                         # bodies change no other output
        assert torch.equal(_bits(out[name]), _bits(plain[name])), name
    assert out["body_count"].shape == (R, 3) and out["body_member_measure"].shape == (R, 3) and out["body_largest_share"].shape == (S, C)
    # the members' measure is the area above the threshold: exceedance_area sums the same layers, unquantised
    models = sections.draw_models(ens, out["draw_slot"])
    area = sections.exceedance_area(models["k"], models["edges"], models["sigma"], x, y, ptr, 0.1, 0.0, Z1_LINES).cpu().numpy()
    width = sections.section_widths(x, y, ptr)
    unit = (width.max() * 1.0) * 2.0 ** -30
    got = out["body_member_measure"].cpu().numpy()
    bound = S * C * unit + (np.diff(ptr) * edges.shape[2])[None, :] * U * area
    print("member measure %.6g .. %.6g m^2, at most %.3g from exceedance_area (bound %.3g)" % (got.min(), got.max(), np.abs(got - area).max(), bound.min()))
    assert area.min() > 0 and np.all(np.abs(got - area) <= bound)
    count, largest = out["body_count"].cpu().numpy(), out["body_largest_measure"].cpu().numpy()
    assert np.all(count >= 1) and np.all(largest <= got) and np.all(largest[count == 1] == got[count == 1])
    share = out["body_largest_share"].cpu().numpy()
    assert share.min() == 0.0 and share.max() == 1.0                           # the top layer never belongs, 60 m always does
    # draw_bodies itself, and its labels against the rule on the first realisations
    b = sections.draw_bodies(ens, out["draw_slot"], depth_edges, x, y, ptr, lo=0.1, log10=False)
    assert torch.equal(b["member_measure"], out["body_member_measure"]) and torch.equal(b["n_bodies"], out["body_count"])
    assert np.array_equal(b["group_ptr"], ptr) and np.array_equal(b["a"], width) and np.array_equal(b["t"], np.ones(C))
    raster = sections.draw_models(ens, out["draw_slot"][:6], depth_edges=depth_edges, log10=False)["raster"].cpu().numpy()
    eu, ev = sections.line_edges(ptr)
    ref = bodies.label_reference(bodies.member_reference(raster, 0.1, np.inf), eu, ev, a=width, t=np.ones(C))
    for name in ("label", "cells", "measure_q"):
        assert np.array_equal(b[name][:6].cpu().numpy(), ref[name]), name
    # on terrain: one elevation axis, NaN outside a sounding's mesh
    from geobipy_amd import elevation
    surface = 100.0 + 4.0 * np.sin(np.arange(S) / 3.0)
    hill = sections.draw_bodies(ens, out["draw_slot"][:4], depth_edges, x, y, ptr, lo=-1.0, surface=surface)
    axis = elevation.regular_axis(surface, depth_edges, 1.0)
    logs = sections.draw_models(ens, out["draw_slot"][:4], depth_edges=depth_edges)["raster"]
    on_axis = elevation.resample(logs.permute(1, 0, 2).contiguous(), surface, depth_edges, edges=axis).permute(1, 0, 2).cpu().numpy()
    assert np.isnan(on_axis).any() and np.array_equal(hill["t"], np.diff(axis))
    ref = bodies.label_reference(bodies.member_reference(on_axis, -1.0, np.inf), eu, ev, a=width, t=np.diff(axis))
    for name in ("label", "cells", "measure_q"):
        assert np.array_equal(hill[name].cpu().numpy(), ref[name]), name
    with pytest.raises(ValueError, match="they need draws >= 1"):
        sections.sections(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, bodies=dict(depth_edges=depth_edges))
    with pytest.raises(ValueError, match="bodies is a dictionary with depth_edges"):
        sections.sections(ens, x, y, Z1_LINES, bodies=dict(depth_edges=depth_edges, threshold=1.0), **kw)


def test_across_lines_the_middle_conductor_joins_its_neighbours_more_often():
    ens, k, edges, sigma, x, y, ptr = _planted()
    S, n = k.shape
    R = 64
    window = np.arange(25.0, 49.0, 1.0)                                        # above the decoy's conductor (from 49 m down), inside the true one
    bd = dict(depth_edges=window, lo=-1.0)
    kw = dict(ptr=ptr, max_models=n, max_distance=1.5 * SPACING, draws=R, seed=2)
    plain = sections.spatial(ens, x, y, Z1_LINES, **kw)
    out = sections.spatial(ens, x, y, Z1_LINES, bodies=bd, **kw)
    assert set(out) == set(plain) | NEW and not NEW & set(plain)
    for name in plain:
        assert torch.equal(_bits(out[name]), _bits(plain[name])), name
    assert out["body_count"].shape == (R, 1) and out["body_largest_share"].shape == (S, window.size - 1)
    alone = sections.spatial(ens, x, y, Z1_LINES, draw_sweeps=0, bodies=bd, **kw)
    eu, ev = out["edge_u"].cpu().numpy(), out["edge_v"].cpu().numpy()
    centre, column = S_LINES + S_LINES // 2, 20                                # 45 m under the centre of the middle line
    a_cell, b_cell = [(centre, column)] * 2, [(centre - S_LINES, column), (centre + S_LINES, column)]

    def joined(res):
        b = sections.draw_bodies(ens, res["draw_slot"], window, x, y, ptr, lo=-1.0, eu=eu, ev=ev)
        return bodies.connected(b, a_cell, b_cell)["probability"].cpu().numpy(), b

    across, b = joined(out)
    apart, _ = joined(alone)
    print("the middle line's conductor joined to its neighbours': across lines %s, line by line %s" % (across, apart))
    assert np.all(across > apart)
    assert torch.equal(b["member_measure"], out["body_member_measure"])
    r = bodies.reach(b, [(centre - S_LINES, column)])
    assert r["share"].shape == (1, S, window.size - 1) and float(r["share"][0, centre, column]) == across[0] and float(r["seed_member"][0]) == 1.0
    with pytest.raises(ValueError, match="they need draws"):
        sections.spatial(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, max_distance=1.5 * SPACING, bodies=bd)


def test_the_command_line_with_bodies(tmp_path, capsys):
    _, k, edges, sigma, x, y, ptr = _planted()
    survey = dict(ensemble_k=k, ensemble_edges=edges, ensemble_sigma=sigma, line=np.repeat([10, 20, 30], S_LINES), x=x, y=y, fiducial=np.arange(k.shape[0]))
    path = str(tmp_path / "survey.npz")
    np.savez(path, **survey)
    bd = dict(depth_edges=np.arange(25.0) * 5.0, lo=-1.0, hi=0.0)
    common = [path, "--depth", "120", "--max-models", "16", "--seed", "3", "--depth-axis", "24", "5"]
    lines = sections.load(sections.main(common + ["--draws", "4", "--bodies", "-1", "0"]))
    without = sections.load(sections.main(common + ["--draws", "4"]))
    direct = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, draws=4, seed=3, bodies=bd))
    assert set(lines) == set(without) | NEW and all(np.array_equal(lines[name], without[name], equal_nan=True) for name in without)
    assert all(np.array_equal(lines[name], direct[name]) for name in NEW) and lines["body_count"].shape == (4, 3) and lines["body_largest_share"].shape == (24, 24)
    graph = sections.load(sections.main(common + ["--spatial", "150", "--spatial-draws", "4", "--bodies", "-1", "0"]))
    direct = _numpy(sections.spatial_from_survey(survey, Z1_LINES, max_models=16, max_distance=150.0, draws=4, seed=3, bodies=bd))
    assert NEW <= set(graph) and all(np.array_equal(graph[name], direct[name]) for name in NEW) and graph["body_count"].shape == (4, 1)
    for argv in (common + ["--bodies", "-1", "0"], common + ["--spatial", "150", "--bodies", "-1", "0"]):
        with pytest.raises(SystemExit):
            sections.main(argv)
        assert "--bodies labels joint realisations: it needs --draws R" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sections.main([path, "--depth", "120", "--draws", "4", "--bodies", "-1", "0"])
    assert "--bodies needs --depth-axis" in capsys.readouterr().err
