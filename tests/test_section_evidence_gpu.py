"""The evidence of the lateral coupling tau on the device (csrc/gbp_section_evidence.h k_section_evidence; geobipy_amd.sections
evidence, fit_tau).

The line entry is held to ``sections.evidence_reference``.  Per output array and rung t the bound is
    max(16 max |fp64 rule - long-double rule|, 16 * 2^-52 * steps * 2^t * max(1, max |value|)),
the maxima over the sequences of the launch, ``steps`` those of its longest sequence (at least 1): 16 is the project's factor
(DESIGN.md 3.25), 2^t the relative error the t squarings of a weight can add.  The inputs keep every step's z far above 1e-280 (the
largest cost of the top rung is 128 * 3 * 1 = 384, exp(-384) = 1e-167), so every value is compared; the rung that certainly
underflows has a test of its own.  Every case prints used / bound."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, sections
from test_families_gpu import _to_device
from test_rjmcmc_gpu import GOLDEN
from test_section_evidence import planted_walk, underflow_chain
from test_spatial_sections import SPACING, Z1_LINES, graph_inputs, lattice_graph, planted_lines, star_graph

U = 2.0 ** -52
SIZES = [1, 2, 63, 64, 65, 128, 257, 1024]
LENGTHS = (1, 2, 40)                                                           # the sequences of one launch


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def _launch(n):
    """Sequences of 1, 2 and 40 soundings with ragged n_used (a 1, an n - 1 and an n among them), NaN outside the prefixes of d2 and of
    score; d2 in [0, 1), g in 0.5 .. 3.  The host arrays and their copies on the device."""
    rng = np.random.default_rng(1000 + n)
    total = sum(LENGTHS)
    nu = rng.choice(np.unique([1, max(n // 3, 1), max(n - 1, 1), n]), total).astype(np.int32)
    nu[0], nu[3:6] = n, (n, n, 1)                                              # a full sequence of one, a full step, a step onto one state
    d2 = np.full((total, n, n), np.nan)
    score = np.full((total, n), np.nan)
    for s in range(total):
        score[s, :nu[s]] = rng.normal(0.0, 1.0, nu[s])
        if s + 1 < total:
            d2[s, :nu[s], :nu[s + 1]] = rng.random((nu[s], nu[s + 1])) ** 2
    g = rng.uniform(0.5, 3.0, total)
    ptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    dev = _dev()
    return ptr, score, g, d2, nu, torch.as_tensor(d2).to(dev), torch.as_tensor(score).to(dev)


@functools.lru_cache(maxsize=None)
def _rule(n, with_score):
    """The rule in fp64 and in long double for the most rungs any launch of n states takes; rung t does not depend on T."""
    ptr, score, g, d2, nu = _launch(n)[:5]
    T = max(t for t in (1, 3, 8) if t * n <= 2048)
    return tuple(sections.evidence_reference(ptr, score if with_score else None, g, d2, nu, T=T, dtype=dt) for dt in (np.float64, np.longdouble))


@pytest.mark.parametrize("with_score", [False, True])
@pytest.mark.parametrize("n,T", [(n, T) for n in SIZES for T in (1, 3, 8) if T * n <= 2048])
def test_line_entry_against_the_rule(n, T, with_score):
    ptr, score, g, d2, nu, d2_dev, score_dev = _launch(n)
    got = sections.evidence(d2_dev, g, ptr, nu, score=score_dev if with_score else None, rungs=T)
    again = sections.evidence(d2_dev, torch.as_tensor(g).to(_dev()), ptr, torch.as_tensor(nu).to(_dev()), score=score_dev if with_score else None, rungs=T)
    r64, rld = _rule(n, with_score)
    steps = max(LENGTHS) - 1
    for name in ("log_partition", "dlog_partition"):
        assert got[name].shape == (T, len(LENGTHS)) and got[name].dtype == np.float64
        assert np.array_equal(_bits(got[name]), _bits(again[name])), name      # a second call, bit for bit
        assert np.all(np.isfinite(got[name]))
        for t in range(T):
            want = rld[name][t]
            bound = max(16.0 * float(np.max(np.abs(r64[name][t] - want))), 16.0 * U * steps * 2.0 ** t * max(1.0, float(np.max(np.abs(want)))))
            used = float(np.max(np.abs(got[name][t] - want)))
            print("n %d T %d %s rung %d: used %.3g bound %.3g" % (n, T, name, t, used, bound))
            assert used <= bound, (name, t, used, bound)
    assert np.all(got["dlog_partition"][:, 0] == 0.0)                          # one sounding: no step, no cost
    assert np.array_equal(got["rank"], np.array(LENGTHS) - 1)


def test_a_long_ladder_is_split_into_launches():
    ptr, score, g, d2, nu, d2_dev, score_dev = _launch(257)
    got = sections.evidence(d2_dev, g, ptr, nu, score=score_dev, tau0=0.4, rungs=9, scale=0.25)      # 7 rungs, then 2: both take their own exp
    want = sections.evidence_reference_ladder(d2, g, ptr, nu, score=score, tau0=0.4, rungs=9, scale=0.25, dtype=np.longdouble)
    fp64 = sections.evidence_reference_ladder(d2, g, ptr, nu, score=score, tau0=0.4, rungs=9, scale=0.25)
    assert np.array_equal(got["tau"], want["tau"]) and np.array_equal(got["scale"], want["scale"]) and np.array_equal(got["rank"], want["rank"])
    steps = max(LENGTHS) - 1
    for name in ("log_partition", "dlog_partition", "log_evidence"):
        for t in range(9):
            rung = t if t < 7 else t - 7                                       # squarings since the launch's own exp
            bound = max(16.0 * float(np.max(np.abs(fp64[name][t] - want[name][t]))),
                        16.0 * U * steps * 2.0 ** rung * max(1.0, float(np.max(np.abs(want[name][t])))))
            assert float(np.max(np.abs(got[name][t] - want[name][t]))) <= bound, (name, t)


def test_the_largest_launch_and_one_state_more():
    lib, dev = _lib.load(), _dev()
    for n, T, ok in ((256, 8, True), (257, 8, False), (1024, 2, True), (1024, 3, False), (683, 3, False), (682, 3, True)):
        total, L = 2, 1
        ptr = torch.tensor([0, 2], dtype=torch.int64, device=dev)
        nu = torch.full((total,), n, dtype=torch.int32, device=dev)
        score, g, d2 = (torch.zeros(shape, dtype=torch.float64, device=dev) for shape in ((total, n), (total,), (total, n, n)))
        lz, dlz = (torch.full((T, L), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
        if ok:
            _lib.call("gbp_section_evidence", dev, L, ptr, total, n, nu, score, g, d2, T, lz, dlz)
            torch.cuda.synchronize()
            assert torch.allclose(lz, torch.full_like(lz, 2.0 * np.log(n)), rtol=0, atol=1e-12) and torch.all(dlz == 0.0)      # no cost at all: Z = n^2
        else:
            with pytest.raises(_lib.NativeLibraryError, match="gbp_section_evidence: T \\* n must not exceed 2048"):
                _lib.call("gbp_section_evidence", dev, L, ptr, total, n, nu, score, g, d2, T, lz, dlz)
            torch.cuda.synchronize()
            assert torch.all(lz == 7.0) and torch.all(dlz == 7.0)


def test_the_rung_that_underflows_is_not_finite_on_the_device_either():
    ptr, score, g, d2, nu = underflow_chain()
    dev = _dev()
    got = sections.evidence(torch.as_tensor(d2).to(dev), g, ptr, nu, score=torch.as_tensor(score).to(dev), rungs=4)
    want = sections.evidence_reference(ptr, score, g, d2, nu, T=4)
    for name in ("log_partition", "dlog_partition"):
        assert np.array_equal(np.isfinite(got[name]), np.isfinite(want[name])), name
        assert np.all(np.isfinite(got[name][:2])) and not np.any(np.isfinite(got[name][2:]))
        assert np.max(np.abs(got[name][:2] - want[name][:2])) <= 16.0 * U * 2 * 2.0 * max(1.0, float(np.max(np.abs(want[name][:2]))))


def test_no_sequence_and_empty_sequences():
    dev = _dev()
    none = sections.evidence(torch.zeros((0, 3, 3), dtype=torch.float64, device=dev), np.zeros(0), np.array([0]), np.zeros(0, dtype=np.int32), rungs=2)
    assert none["log_partition"].shape == (2, 0) and none["log_evidence"].shape == (2, 0)
    ptr, score, g, d2, nu, d2_dev, score_dev = _launch(2)
    cut = np.array([0, 1, 1, 3, 3, ptr[-1]], dtype=np.int64)                   # sequences of 1, 0, 2, 0 and 40 soundings
    got = sections.evidence(d2_dev, g, cut, nu, score=score_dev, rungs=3)
    want = sections.evidence_reference_ladder(d2, g, cut, nu, score=score, rungs=3)
    assert np.array_equal(got["rank"], [0, 0, 1, 0, 39]) and np.all(got["log_partition"][:, [1, 3]] == 0.0) and np.all(got["log_evidence"][:, [1, 3]] == 0.0)
    assert np.allclose(got["log_evidence"], want["log_evidence"], rtol=0, atol=1e-10)


def test_fit_on_the_device_against_the_fit_on_the_rules():
    y, x, ptr, g, d2, nu = planted_walk(0)
    dev_fit = sections.fit_tau(torch.as_tensor(d2).to(_dev()), g, ptr, nu)
    rule_fit = sections.fit_tau_reference(d2, g, ptr, nu)
    print("device %.6f rule %.6f sd_log %.4f / %.4f" % (dev_fit["tau"], rule_fit["tau"], dev_fit["tau_sd_log"], rule_fit["tau_sd_log"]))
    assert dev_fit["bracketed"] and dev_fit["bracket"] == rule_fit["bracket"] and dev_fit["rank"] == rule_fit["rank"]
    assert abs(np.log(dev_fit["tau"] / rule_fit["tau"])) <= 4e-3              # two refinement tolerances
    assert np.allclose(dev_fit["log_evidence"], rule_fit["log_evidence"], rtol=1e-9, atol=1e-7) and dev_fit["tau_sd_log"] > 0.0
    short = sections.fit_tau(torch.as_tensor(d2).to(_dev()), g, ptr, nu, rungs=3)
    assert short["bracketed"] is False and np.isnan(short["tau_sd_log"]) and abs(short["tau"] - 0.4) < 1e-12


def test_evidence_refuses_what_is_not_on_the_device_or_badly_shaped():
    ptr, score, g, d2, nu, d2_dev, score_dev = _launch(2)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_evidence"):
        sections.evidence(d2, g, ptr, nu)                                    # numpy: there is no host fallback
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_evidence"):
        sections.evidence(d2_dev.cpu(), g, ptr, nu)
    with pytest.raises(TypeError, match="float64"):
        sections.evidence(d2_dev.float(), g, ptr, nu)
    with pytest.raises(ValueError, match="rungs"):
        sections.evidence(d2_dev, g, ptr, nu, rungs=0)
    with pytest.raises(ValueError, match="tau_max"):
        sections.fit_tau(d2_dev, g, ptr, nu, tau_max=-1.0)


def test_the_c_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    total, L, n, T = 3, 2, 5, 3
    ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device=dev)
    nu = torch.full((total,), n, dtype=torch.int32, device=dev)
    score, g, d2 = (torch.zeros(shape, dtype=torch.float64, device=dev) for shape in ((total, n), (total,), (total, n, n)))
    lz, dlz = (torch.full((T, L), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
    p = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    call = lambda L_=L, ptr_=ptr, total_=total, n_=n, nu_=nu, score_=score, g_=g, d2_=d2, T_=T, lz_=lz, dlz_=dlz: \
        lib.gbp_section_evidence(L_, p(ptr_), total_, n_, p(nu_), p(score_), p(g_), p(d2_), T_, p(lz_), p(dlz_), st)      # noqa: E731
    for kw in (dict(L_=-1), dict(n_=0), dict(n_=1025), dict(T_=0), dict(T_=9), dict(T_=-1), dict(n_=1024, T_=3), dict(total_=1), dict(total_=2 ** 62),
               dict(ptr_=None), dict(nu_=None), dict(score_=None), dict(g_=None), dict(d2_=None), dict(lz_=None), dict(dlz_=None), dict(L_=0, T_=9)):
        assert call(**kw) != 0 and b"gbp_section_evidence" in lib.gbp_last_error(), kw
    assert call(L_=0, ptr_=None) == 0                                          # no sequence: OK without a launch
    torch.cuda.synchronize()
    assert torch.all(lz == 7.0) and torch.all(dlz == 7.0)                      # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    want = torch.tensor([np.log(n), 2.0 * np.log(n)], dtype=torch.float64, device=dev).expand(T, L)
    assert torch.allclose(lz, want, rtol=0, atol=1e-14) and torch.all(dlz == 0.0)      # no cost at all: Z = n and n^2


# ---- the survey graph ----------------------------------------------------------------------------------------------------------------

def _graph_case(name, n):
    """eu, ev, n_used (ragged, with a 1 and an n), score, g, d2 of a named graph; the planted lines come with their own distances."""
    rng = np.random.default_rng(500 + 7 * n + len(name))
    if name == "tree":
        eu, ev, _ = star_graph()
        S = 5
    elif name == "lattice":
        eu, ev, S = lattice_graph(3, 3)
    elif name == "isolated":                                                   # sounding 2 has no edge; 5 neither, at the end
        eu, ev, S = np.array([0, 0, 1, 3]), np.array([1, 3, 4, 4]), 6
    else:                                                                      # no edge at all
        eu, ev, S = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 3
    nu = rng.integers(1, n + 1, S)
    nu[0], nu[S - 2] = n, 1
    score, g, d2 = graph_inputs(rng, eu, ev, nu, n)
    return eu, ev, nu, score, g * 0.1, d2                                      # (a tenth of the couplings of graph_inputs: beliefs that stay spread out)


def _check_terms(what, got, r64, rld):
    """The entry's three arrays against the rule on the same messages: the bound of the module's docstring with one step and rung 0."""
    for name in ("node_log_z", "edge_log_z", "edge_energy"):
        want = rld[name]
        assert got[name].shape == want.shape and np.all(np.isfinite(got[name]))
        if not want.size:
            continue
        bound = max(16.0 * float(np.max(np.abs(r64[name] - want))), 16.0 * U * max(1.0, float(np.max(np.abs(want)))))
        used = float(np.max(np.abs(got[name] - want)))
        print("%s %s: used %.3g bound %.3g" % (what, name, used, bound))
        assert used <= bound, (what, name, used, bound)


@pytest.mark.parametrize("n", [3, 64, 65, 256])
@pytest.mark.parametrize("name", ["tree", "lattice", "isolated", "no edges"])
def test_graph_entry_against_its_rule(name, n):
    eu, ev, nu, score, g, d2 = _graph_case(name, n)
    dev, S = _dev(), nu.size
    d2_dev, score_dev = torch.as_tensor(d2).to(dev), torch.as_tensor(score).to(dev)
    plain = sections.propagate(d2_dev, g, eu, ev, nu, S, score=score_dev, sweeps=6)
    kept = sections.propagate(d2_dev, g, eu, ev, nu, S, score=score_dev, sweeps=6, keep_messages=True)
    assert set(kept) == set(plain) | {"message", "node_weight"}
    for key in plain:
        assert torch.equal(plain[key], kept[key]), key                         # the keyword changes no bit of what was there
    assert kept["message"].shape == (2 * eu.size, n) and kept["node_weight"].shape == (S, n)
    got = {k: v.cpu().numpy() for k, v in sections.graph_terms(d2_dev, g, eu, ev, nu, S, kept["node_weight"], kept["message"]).items()}
    again = {k: v.cpu().numpy() for k, v in sections.graph_terms(d2_dev, g, eu, ev, nu, S, kept["node_weight"], kept["message"]).items()}
    assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got)    # a second call, bit for bit
    w, msg = kept["node_weight"].cpu().numpy(), kept["message"].cpu().numpy()
    r64 = sections.graph_terms_reference(eu, ev, g, d2, nu, w, msg)
    rld = sections.graph_terms_reference(eu, ev, g, d2, nu, w, msg, dtype=np.longdouble)
    _check_terms("%s n=%d" % (name, n), got, r64, rld)
    # the whole of it against the rule's own message passing: the messages differ by their own rounding, sweep after sweep
    dev_ev = sections.graph_evidence(d2_dev, g, eu, ev, nu, S, score=score_dev, sweeps=6)
    e64 = sections.graph_evidence_reference(eu, ev, g, d2, nu, score, sweeps=6)
    eld = sections.graph_evidence_reference(eu, ev, g, d2, nu, score, sweeps=6, dtype=np.longdouble)
    assert dev_ev["rank"] == e64["rank"] == sections.graph_rank(eu, ev, S)
    for key in ("log_partition", "dlog_partition", "log_evidence"):
        bound = max(16.0 * abs(float(e64[key] - eld[key])), 16.0 * U * 6 * max(1.0, abs(float(eld[key]))))
        print("%s n=%d %s: used %.3g bound %.3g" % (name, n, key, abs(dev_ev[key] - float(eld[key])), bound))
        assert abs(dev_ev[key] - float(eld[key])) <= bound, key
    if name == "no edges":
        assert dev_ev["dlog_partition"] == 0.0 and dev_ev["edge_energy"].shape == (0,) and abs(dev_ev["log_evidence"]) <= 64 * U


def test_graph_evidence_on_the_planted_lines():
    k, edges, sigma, x, y, ptr, _ = planted_lines()
    ens = _to_device(k, edges, sigma)
    S, n = k.shape
    rows = torch.arange(n, dtype=torch.int32, device=_dev())[None, :].repeat(S, 1)
    nu = np.full(S, n)
    eu, ev, g, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * SPACING, tau=0.4)
    assert eu.size == 37 and sections.graph_rank(eu, ev, S) == S - 1
    d2_dev = sections.edge_distance(ens, rows, eu, ev, 0.0, Z1_LINES)
    d2 = d2_dev.cpu().numpy()
    kept = sections.propagate(d2_dev, g, eu, ev, nu, S, sweeps=32, keep_messages=True)
    got = {name: v.cpu().numpy() for name, v in sections.graph_terms(d2_dev, g, eu, ev, nu, S, kept["node_weight"], kept["message"]).items()}
    w, msg = kept["node_weight"].cpu().numpy(), kept["message"].cpu().numpy()
    _check_terms("planted lines", got, sections.graph_terms_reference(eu, ev, g, d2, nu, w, msg),
                 sections.graph_terms_reference(eu, ev, g, d2, nu, w, msg, dtype=np.longdouble))
    whole = sections.graph_evidence(d2_dev, g, eu, ev, nu, S, sweeps=32)
    assert whole["residual"][-1] < 1e-6 and whole["edge_energy"].shape == (37,) and np.all(whole["edge_energy"] >= 0.0)
    assert abs(whole["dlog_partition"] + got["edge_energy"].sum()) <= 1e-12 * max(1.0, abs(whole["dlog_partition"]))
    fit = sections.fit_tau_graph(d2_dev, g, eu, ev, nu, S, tau0=0.4, sweeps=32)
    print("planted lines: tau %.4f bracketed %r residual %s" % (fit["tau"], fit["bracketed"], fit["residual"]))
    assert fit["residual"].shape == (11,) and fit["tau_ladder"].shape == (11,) and fit["rank"] == S - 1
    assert 0.025 <= fit["tau"] <= 0.8 and fit["edge_energy"].shape == (11, 37)


def test_the_graph_entry_refuses_bad_arguments_by_name():
    lib, dev = _lib.load(), _dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    S, E, n = 3, 2, 4
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)             # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)      # noqa: E731
    eu, ev, nu, in_ptr, in_edge = i32([0, 1]), i32([1, 2]), i32([4, 4, 4]), i32([0, 1, 3, 4]), i32([1, 0, 3, 2])
    w, g, d2, msg, node, edge, energy = f64(S, n), f64(E), f64(E, n, n), f64(2 * E, n), f64(S), f64(E), f64(E)
    p = lambda a: None if a is None else a.data_ptr()                          # noqa: E731
    call = lambda S_=S, E_=E, n_=n, eu_=eu, ev_=ev, nu_=nu, w_=w, g_=g, d2_=d2, ptr_=in_ptr, edge_=in_edge, msg_=msg, node_=node, lz_=edge, en_=energy: \
        lib.gbp_section_graph_evidence(S_, E_, n_, p(eu_), p(ev_), p(nu_), p(w_), p(g_), p(d2_), p(ptr_), p(edge_), p(msg_), p(node_), p(lz_), p(en_), st)      # noqa: E731
    for kw in (dict(S_=-1), dict(E_=-1), dict(E_=2 ** 30), dict(n_=0), dict(n_=257), dict(S_=1), dict(S_=2 ** 31 - 1, E_=2 ** 29), dict(eu_=None),
               dict(ev_=None), dict(nu_=None), dict(w_=None), dict(g_=None), dict(d2_=None), dict(ptr_=None), dict(edge_=None), dict(msg_=None),
               dict(node_=None), dict(lz_=None), dict(en_=None)):
        assert call(**kw) != 0 and b"gbp_section_graph_evidence" in lib.gbp_last_error(), kw
    assert call(S_=0, E_=0, nu_=None, w_=None, ptr_=None, node_=None) == 0     # nothing: OK without a launch
    torch.cuda.synchronize()
    for t in (node, edge, energy):
        assert bool((t == 7.0).all())                                          # nothing was written
    with pytest.raises(ValueError, match="node_weight"):
        sections.graph_terms(d2, g, eu, ev, nu, S, w[:2], msg)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_section_graph_evidence"):
        sections.graph_terms(d2.cpu(), g, eu, ev, nu, S, w.cpu(), msg.cpu())


# ---- a survey and the command line -----------------------------------------------------------------------------------------------------

def test_fit_from_survey_and_the_command_line(tmp_path, capsys):
    from geobipy_amd import survey
    res = survey.infer(os.path.join(GOLDEN, "resolve_options_small"), exact_jacobian=True, ensemble=16)
    path = str(tmp_path / "survey.npz")
    res.save(path)
    z1 = 120.0
    fit = sections.fit_from_survey(path, z1, z0=2.0, measure="log", max_models=16)
    assert fit["tau_ladder"].shape == (11,) and fit["log_evidence"].shape == (11,) and 0.025 <= fit["tau"] <= 0.8 and fit["rank"] > 0
    assert fit["bracketed"] == bool(np.isfinite(fit["tau_sd_log"]))
    written = sections.main([path, "--depth", "120", "--from", "2", "--measure", "log", "--max-models", "16", "--fit-tau"])
    printed = capsys.readouterr().out
    assert "fit: tau = %.4g" % fit["tau"] in printed and ("bracketed" in printed)
    f = sections.load(written)
    assert float(f["fit_tau"]) == fit["tau"] and np.array_equal(f["fit_tau_ladder"], fit["tau_ladder"])
    assert np.array_equal(f["fit_log_evidence"], fit["log_evidence"], equal_nan=True)      # (a rung whose weights underflow is NaN, and skipped)
    assert np.array_equal(f["fit_tau_sd_log"], np.float64(fit["tau_sd_log"]), equal_nan=True)
    direct = sections.from_survey(path, z1, z0=2.0, measure="log", max_models=16, tau=fit["tau"])      # tau_hat serves everything else
    for name, v in direct.items():
        assert np.array_equal(f[name], v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v), equal_nan=True), name
    assert set(f) == set(direct) | {"fit_tau", "fit_tau_sd_log", "fit_tau_ladder", "fit_log_evidence"}
    plain = sections.load(sections.main([path, "--depth", "120", "--from", "2", "--measure", "log", "--max-models", "16"]))
    assert not any(name.startswith("fit_") for name in plain)                  # without --fit-tau nothing changes: tau = 0.1
    default = sections.from_survey(path, z1, z0=2.0, measure="log", max_models=16)
    assert all(np.array_equal(plain[name], v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v), equal_nan=True) for name, v in default.items())
    short = sections.load(sections.main([path, "--depth", "120", "--max-models", "16", "--fit-tau", "0.8", "2"]))
    assert short["fit_tau_ladder"].shape == (2,)
    across = sections.load(sections.main([path, "--depth", "120", "--max-models", "16", "--spatial", "500", "--sweeps", "8", "--fit-tau", "0.8", "5"]))
    assert across["fit_tau_ladder"].shape == (5,) and 0.8 / 4.0 - 1e-12 <= float(across["fit_tau"]) <= 0.8 and "residual" in across
    for argv in (["--fit-tau", "--tau", "0.2"], ["--tau", "0.2", "--fit-tau", "0.8"], ["--fit-tau", "0.8", "1"], ["--fit-tau", "-1"],
                 ["--fit-tau", "0.8", "2.5"], ["--fit-tau", "0.8", "5", "7"]):
        with pytest.raises(SystemExit):
            sections.parse_args([path, "--depth", "120"] + argv)
    assert "--fit-tau learns tau: it is not given together with --tau" in capsys.readouterr().err
