"""The most probable section across flight lines, the rule alone (geobipy_amd.sections graph_path_reference, refine_reference,
decode_levels, sounding_colours): no GPU.

The rule is held to what it must equal where that is known: enumeration of every configuration on trees, ``track_reference``'s
Viterbi path on a line, and on a small lattice with loops -- where it is an approximation -- to the properties that hold by
construction.  A comparison with an enumerated mode is made only where the enumerated gap to the runner-up is at least GAP = 1e-9
(below it the two orders of summation may rank them differently); every test prints how many cases that left out."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from geobipy_amd import _lib, sections
from test_spatial_sections import (S_LINES, SPACING, Z1_LINES, edge_distance_reference, graph_inputs, lattice_graph, line_graph, planted_lines,
                                   star_graph)

GAP = 1e-9


def log_scores(X, score, g, d2, eu, ev):
    return sections._host_log_score(np.atleast_2d(np.asarray(X, dtype=np.int32)), score, g, d2, eu, ev)


def enumerate_mode(eu, ev, g, d2, n_used, score):
    """The most probable configuration by enumeration, its log score and the gap to the runner-up."""
    cfgs = np.array(list(itertools.product(*[range(m) for m in n_used])), dtype=np.int32)
    ls = log_scores(cfgs, score, g, d2, eu, ev)
    order = np.argsort(-ls, kind="stable")
    return cfgs[order[0]], ls[order[0]], ls[order[0]] - ls[order[1]]


# ---- trees: exact ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,diameter", [("line", 5), ("star", 3)])
def test_trees_against_every_configuration(name, diameter):
    eu, ev, n_used = line_graph() if name == "line" else star_graph()
    n_used = np.minimum(n_used, 5)
    left_out = 0
    for seed in range(20):
        score, g, d2 = graph_inputs(np.random.default_rng(100 + seed), eu, ev, n_used, 5)
        mode, best, gap = enumerate_mode(eu, ev, g, d2, n_used, score)
        got = sections.graph_path_reference(eu, ev, g, d2, n_used, score, sweeps=diameter + 3)
        assert np.all(got["residual"][diameter:] == 0.0) and np.all(got["residual"][:2] > 0.0)      # every message has its final bits
        assert np.all(got["refine_moves"] == 0) and got["chosen"] == 0        # a mode: no single move raises the score
        assert got["state"].dtype == np.int32 and got["decoded_state"].dtype == np.int32 and got["refine_moves"].shape == (1, 16)
        for s in range(n_used.size):                                          # max-marginals: 0.0 at the mode, -inf beyond the prefix
            assert np.all(got["max_marginal"][s, n_used[s]:] == -np.inf) and got["max_marginal"][s, :n_used[s]].max() == 0.0
        if gap < GAP:
            left_out += 1
            continue
        assert np.array_equal(got["decoded_state"], mode) and np.array_equal(got["state"], mode), (name, seed)
        assert abs(got["log_score"] - best) <= 1e-12
        # the max-marginal is the log probability lost by forcing a sounding onto a model: against the enumeration, sounding 0
        for i in range(n_used[0]):
            forced = [range(m) for m in n_used]
            forced[0] = [i]
            cfgs = np.array(list(itertools.product(*forced)), dtype=np.int32)
            assert abs(got["max_marginal"][0, i] - (log_scores(cfgs, score, g, d2, eu, ev).max() - best)) <= 1e-10
    print("%s: %d of 20 draws left out (gap to the runner-up below %g)" % (name, left_out, GAP))
    assert left_out <= 1                                                      # at most 5 %


def test_a_line_against_viterbi():
    eu, ev, n_used = line_graph()
    S, n, left_out = n_used.size, 5, 0
    for seed in range(20):
        rng = np.random.default_rng(200 + seed)
        score, g, d2 = rng.normal(size=(S, n)), rng.uniform(5.0, 60.0, S), rng.uniform(0.0, 0.3, (S, n, n))
        _, _, gap = enumerate_mode(eu, ev, g[:-1], d2[:-1], n_used, score)
        if gap < GAP:
            left_out += 1
            continue
        chain = sections.track_reference([0, S], score, g, d2, n_used, marginals=False)
        got = sections.graph_path_reference(eu, ev, g[:-1], d2[:-1], n_used, score, sweeps=6)
        assert np.array_equal(got["state"], chain["state"]), seed
        assert abs(got["log_score"] - float(np.asarray(chain["log_score"]).reshape(-1)[0])) <= 1e-12
    print("line against Viterbi: %d of 20 draws left out" % left_out)
    assert left_out <= 1


def test_a_planted_tie_is_not_mixed():
    """Three soundings in a path, state 1 a duplicate of state 0 everywhere but for the cost of changing between them: the sections
    (0, 0, 0) and (1, 1, 1) are exactly equal modes, every sum being one of small integers.  The argmax of the max-marginals sounding
    by sounding cannot tell them apart; conditioning level by level returns one of them whole."""
    eu, ev, n_used = np.array([0, 1]), np.array([1, 2]), np.array([3, 3, 3])
    score = np.array([[2.0, 2.0, 0.0], [1.0, 1.0, 0.0], [3.0, 3.0, 1.0]])
    one = np.array([[0.0, 4.0, 5.0], [4.0, 0.0, 5.0], [6.0, 6.0, 0.0]])
    g, d2 = np.array([1.0, 2.0]), np.stack([one, one])
    mode, best, gap = enumerate_mode(eu, ev, g, d2, n_used, score)
    assert gap == 0.0 and best == 6.0
    assert log_scores([[0, 0, 0], [1, 1, 1], [0, 1, 1], [1, 0, 0]], score, g, d2, eu, ev).tolist() == [6.0, 6.0, 2.0, 2.0]
    for sweeps in (2, 5):
        got = sections.graph_path_reference(eu, ev, g, d2, n_used, score, sweeps=sweeps)
        assert np.all(got["max_marginal"][:, :2] == 0.0) and np.all(got["max_marginal"][:, 2] < 0.0)      # both modes, at every sounding
        assert got["decoded_state"].tolist() == [0, 0, 0] and got["log_score"] == 6.0 and np.all(got["refine_moves"] == 0)
    # the twins of the middle sounding renumbered: the modes are (0, 1, 0) and (1, 0, 1), and the first maxima of the max-marginals,
    # (0, 0, 0), are a mix of the two that pays for a change on both edges: 12 less probable
    swap = [1, 0, 2]
    d2s = np.stack([one[:, swap], one[swap, :]])
    assert log_scores([[0, 1, 0], [1, 0, 1], [0, 0, 0]], score, g, d2s, eu, ev).tolist() == [6.0, 6.0, -6.0]
    got = sections.graph_path_reference(eu, ev, g, d2s, n_used, score, sweeps=3, refine=0)
    assert np.argmax(got["max_marginal"], axis=1).tolist() == [0, 0, 0]
    assert got["decoded_state"].tolist() == [0, 1, 0] and got["state"].tolist() == [0, 1, 0] and got["log_score"] == 6.0


# ---- loops: an approximation with guarantees ------------------------------------------------------------------------------------------

def test_the_lattice_with_loops():
    eu, ev, S = lattice_graph(3, 3)
    n_used = np.full(S, 3)
    modes_path = modes_belief = modes_decode = 0
    worst = 0.0
    for seed in range(40):
        score, g, d2 = graph_inputs(np.random.default_rng(seed), eu, ev, n_used, 3)
        _, best, _ = enumerate_mode(eu, ev, g, d2, n_used, score)
        belief = sections.propagate_reference(eu, ev, g, d2, n_used, score, sweeps=32)["state"]
        got = sections.graph_path_reference(eu, ev, g, d2, n_used, score, sweeps=32, candidates=belief[None, :])
        assert got["candidate_state"].shape == (2, S) and got["refine_moves"].shape == (2, 16)
        # every refine move raises the score: sweep by sweep from both starts
        for start in (got["decoded_state"], belief):
            x, before = start.copy(), log_scores(start, score, g, d2, eu, ev)[0]
            for _ in range(16):
                step = sections.refine_reference(x, eu, ev, g, d2, n_used, score, sweeps=1)
                after = step["log_score"]
                assert (after > before) if step["refine_moves"][0] else (after == before and np.array_equal(step["state"], x))
                x, before = step["state"], after
        assert np.array_equal(x, got["candidate_state"][1])                   # sweep by sweep is the same ascent
        assert got["candidate_log_score"][got["chosen"]] == got["candidate_log_score"].max() == got["log_score"]
        assert got["log_score"] >= log_scores(belief, score, g, d2, eu, ev)[0] and got["log_score"] >= log_scores(got["decoded_state"], score, g, d2, eu, ev)[0]
        assert np.array_equal(got["state"], got["candidate_state"][got["chosen"]])
        assert got["log_score"] <= best + 1e-12
        modes_path += got["log_score"] >= best - 1e-12
        modes_decode += log_scores(got["decoded_state"], score, g, d2, eu, ev)[0] >= best - 1e-12
        modes_belief += log_scores(belief, score, g, d2, eu, ev)[0] >= best - 1e-12
        worst = max(worst, float(best - got["log_score"]))
    print("3 x 3 lattice, 3 states, 40 seeds: exact modes -- belief argmax %d, decode %d, refined and chosen %d; the largest gap to the mode %.3g"
          % (modes_belief, modes_decode, modes_path, worst))
    assert modes_path >= modes_belief and modes_path > modes_belief


def test_the_planted_lines_on_the_rules_alone():
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    S, n = k.shape
    rows, n_used = np.tile(np.arange(n, dtype=np.int32), (S, 1)), np.full(S, n)
    middle = np.arange(S_LINES, 2 * S_LINES)
    # 1.5 line spacings: loops
    eu, ev, g, _ = sections.neighbours(x, y, ptr, n_used, max_distance=1.5 * SPACING)
    d2 = edge_distance_reference(k, edges, sigma, rows, eu, ev, 0.0, Z1_LINES)
    belief = sections.propagate_reference(eu, ev, g, d2, n_used, None, sweeps=32)["state"]
    got = sections.graph_path_reference(eu, ev, g, d2, n_used, None, sweeps=32, candidates=belief[None, :])
    s_belief = log_scores(belief, None, g, d2, eu, ev)[0]
    print("planted lines: belief argmax %.3f, its ascent %.3f, the path %.3f (%d soundings differ); residual %s"
          % (s_belief, got["candidate_log_score"][1], got["log_score"], int((got["state"] != belief).sum()), got["residual"][[0, 7, 15, 31]]))
    assert np.all(got["state"][middle] >= 10) and got["log_score"] > s_belief
    # 0.5 line spacings: a forest, every line its own chain
    eu, ev, g, _ = sections.neighbours(x, y, ptr, n_used, max_distance=0.5 * SPACING)
    d2 = edge_distance_reference(k, edges, sigma, rows, eu, ev, 0.0, Z1_LINES)
    alone = sections.graph_path_reference(eu, ev, g, d2, n_used, None, sweeps=8)
    chain = sections.cross_distance_reference(k, edges, sigma, rows, sections.partners(ptr, n_used), 0.0, Z1_LINES)
    track = sections.track_reference(ptr, None, sections.steps(x, y, ptr=ptr), chain, n_used, marginals=False)["state"]
    assert np.all(alone["residual"][7:] == 0.0) and np.all(alone["refine_moves"] == 0)
    for line in range(3):
        assert np.array_equal(alone["state"][8 * line:8 * line + 8], track[8 * line:8 * line + 8]), line


# ---- host functions and plumbing ------------------------------------------------------------------------------------------------------

def test_levels_and_colours_by_hand():
    eu, ev, _ = star_graph()
    level, level_ptr, level_node = sections.decode_levels(eu, ev, 5)
    assert level.tolist() == [0, 1, 1, 1, 2] and level_ptr.tolist() == [0, 1, 4, 5] and level_node.tolist() == [0, 1, 2, 3, 4]
    assert level.dtype == np.int32 and level_ptr.dtype == np.int32 and level_node.dtype == np.int32
    colour, n_colours = sections.sounding_colours(eu, ev, 5)
    assert colour.tolist() == [0, 1, 1, 1, 0] and n_colours == 2
    eu, ev, S = lattice_graph(3, 3)                                           # level = row + column, colour = its parity
    level, level_ptr, level_node = sections.decode_levels(eu, ev, S)
    assert level.tolist() == [0, 1, 2, 1, 2, 3, 2, 3, 4] and level_ptr.tolist() == [0, 1, 3, 6, 8, 9]
    assert level_node.tolist() == [0, 1, 3, 2, 4, 6, 5, 7, 8]
    colour, n_colours = sections.sounding_colours(eu, ev, S)
    assert colour.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0] and n_colours == 2
    # two pieces and a sounding alone: every piece starts at level 0; a triangle needs three colours
    level, level_ptr, level_node = sections.decode_levels([0, 0, 1, 4], [1, 2, 2, 5], 6)
    assert level.tolist() == [0, 1, 1, 0, 0, 1] and level_ptr.tolist() == [0, 3, 6] and level_node.tolist() == [0, 3, 4, 1, 2, 5]
    assert sections.sounding_colours([0, 0, 1, 4], [1, 2, 2, 5], 6)[0].tolist() == [0, 1, 2, 0, 0, 1]
    none = sections.decode_levels(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0)
    assert none[0].size == 0 and none[1].tolist() == [0] and none[2].size == 0
    for call in (sections.decode_levels, sections.sounding_colours):
        with pytest.raises(ValueError, match="sorted"):
            call([1, 0], [2, 1], 3)
        with pytest.raises(ValueError, match="eu < ev"):
            call([0], [3], 3)


def test_refusals_come_before_the_library():
    d2, g, n_used = torch.zeros((3, 4, 4), dtype=torch.float64), np.ones(3), np.array([4, 1, 2, 4])
    eu, ev = np.array([0, 0, 2]), np.array([1, 3, 3])
    for call in (lambda d2_=d2, **kw: sections.graph_path(d2_, g, eu, ev, n_used, 4, **kw),
                 lambda d2_=d2, **kw: sections.graph_path_reference(eu, ev, g, d2_, n_used, **kw)):
        for kw, match in ((dict(sweeps=0), "sweeps"), (dict(damping=1.0), "damping"), (dict(refine=-1), "refine"), (dict(refine=1.5), "refine"),
                          (dict(candidates=np.zeros((1, 3), dtype=np.int64)), "candidates"), (dict(candidates=np.zeros((1, 4))), "candidates"),
                          (dict(candidates=np.array([[0, 1, 0, 0]])), "n_used - 1"), (dict(candidates=np.array([[0, 0, 0, -1]])), "n_used - 1"),
                          (dict(score=torch.zeros((4, 3), dtype=torch.float64)), "score")):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    for call in (lambda state, **kw: sections.refine(state, d2, g, eu, ev, n_used, **kw),
                 lambda state, **kw: sections.refine_reference(state, eu, ev, g, d2, n_used, **kw)):
        with pytest.raises(ValueError, match="state"):
            call(np.zeros(3, dtype=np.int64))
        with pytest.raises(ValueError, match="n_used - 1"):
            call(np.array([0, 0, 2, 0]))
        with pytest.raises(ValueError, match="sweeps"):
            call(np.zeros(4, dtype=np.int64), sweeps=-1)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.graph_path(d2.numpy(), g, eu, ev, n_used, 4)
    with pytest.raises(_lib.NativeLibraryError, match="no host fallback"):
        sections.refine(np.zeros(4, dtype=np.int64), d2.numpy(), g, eu, ev, n_used)
    with pytest.raises(ValueError, match="n_used"):
        sections.graph_path(d2, g, eu, ev, n_used, 5)
    with pytest.raises(TypeError):
        sections.graph_path(d2.float(), g, eu, ev, n_used, 4)
    with pytest.raises(TypeError):
        sections.refine(np.zeros(4, dtype=np.int64), d2.float(), g, eu, ev, n_used)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_graph_path"):       # host tensors: refused last
        sections.graph_path(d2, g, eu, ev, n_used, 4)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_graph_refine"):
        sections.refine(np.zeros(4, dtype=np.int64), d2, g, eu, ev, n_used)
    assert sections.check_path(None, "x") is None and sections.check_path(True, "x") == dict(sweeps=32, damping=0.0, refine=16)
    assert sections.check_path(dict(sweeps=5, refine=0), "x") == dict(sweeps=5, damping=0.0, refine=0)
    for bad in (dict(sweep=3), dict(sweeps=0), dict(damping=1.0), dict(refine=-1), 3, "yes"):
        with pytest.raises(ValueError):
            sections.check_path(bad, "x")


def test_the_signatures_declare_the_entries():
    assert len(_lib.SIGNATURES["gbp_section_graph_path"][1]) == 23 and len(_lib.SIGNATURES["gbp_section_graph_refine"][1]) == 19
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "geobipy_amd.h")) as f:
        text = f.read()
    for name, count in (("gbp_section_graph_path", 23), ("gbp_section_graph_refine", 19)):
        declaration = text.split("gbp_status %s(" % name)[1].split(");")[0]
        assert len(declaration.split(",")) == count, name


def test_the_command_line_takes_path(capsys):
    base = ["run.npz", "--depth", "150", "--spatial", "300"]
    assert sections.parse_args(base + ["--path"])[1]["path"] is True
    assert sections.parse_args(base + ["--path", "12"])[1]["path"] == dict(sweeps=12)
    assert sections.parse_args(base + ["--path", "--spatial-draws", "4"])[1]["draws"] == 4
    assert "path" not in sections.parse_args(base)[1]
    for argv in (["run.npz", "--depth", "10", "--path"], base + ["--path", "0"], base + ["--path", "x"]):
        with pytest.raises(SystemExit):
            sections.parse_args(argv)
    capsys.readouterr()
