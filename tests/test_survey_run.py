"""The parts of a survey run (geobipy_amd/survey_run.py) on the CPU: the sampler's arguments, the order of the device rows' columns and
the container filler's one thread, with stand-ins for the sampler, the payload and the writer."""
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from geobipy_amd import hdf, survey, survey_run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTIONS = os.path.join(GOLDEN, "resolve_options_small")


def test_sampler_arguments_follow_the_options_and_the_call():
    o = survey.read_options(OPTIONS)
    kw = survey_run.sampler_arguments(o, False, seed=None, device="cpu", hitmap=True, first_chain=7, burn_in_min_iterations=123, containers=True)
    assert kw["seed"] == o["seed"] % (1 << 64) and kw["first_chain"] == 7 and kw["burn_in_min_iterations"] == 123 and kw["reference_schedule"] is True
    assert kw["n_markov_chains"] == 6000 and kw["probability_of_birth"] == 1.0 / 6.0 and kw["factor"] == 10.0 and kw["hitmap"] is True
    assert set(kw) - {"seed", "device", "hitmap", "first_chain", "reference_schedule", "burn_in_min_iterations", "trace_every"} <= set(survey_run.OPTION_KEYS)
    unset = [k for k in survey_run.OPTION_KEYS if o.get(k) is None]      # (an option the file leaves out is left to the sampler's default)
    assert unset and not set(unset) & set(kw) and {k: kw[k] for k in survey_run.OPTION_KEYS if k not in unset} == {k: o[k] for k in survey_run.OPTION_KEYS if k not in unset}
    assert survey_run.sampler_arguments(o, False, seed=-1)["seed"] == (1 << 64) - 1
    # traces: kept only when containers are written -- 1: the full arrays; "auto": the smallest stride with at most 4 096 entries; None: none
    assert kw["trace_every"] == 1
    assert survey_run.sampler_arguments(o, False, containers=True, traces="auto")["trace_every"] == 3          # 12 000 entries / 4 096
    assert survey_run.sampler_arguments(dict(o, n_markov_chains=2000), False, containers=True, traces="auto")["trace_every"] == 1
    assert survey_run.sampler_arguments(o, False, containers=True, traces=8)["trace_every"] == 8
    assert "trace_every" not in survey_run.sampler_arguments(o, False, containers=True, traces=None)
    assert "trace_every" not in survey_run.sampler_arguments(o, False, containers=False, traces=1)
    # hankel_eps: ppm for frequency-domain data, relative for time-domain data; absent when not given
    fd = survey_run.sampler_arguments(o, False, hankel_eps=0)
    assert fd["hankel_eps_ppm"] == 0.0 and isinstance(fd["hankel_eps_ppm"], float) and "hankel_eps" not in fd
    ot = survey.read_options(os.path.join(GOLDEN, "tempest_options_small"))
    td = survey_run.sampler_arguments(dict(ot, solve_receiver_pitch=True, maximum_receiver_pitch_change=5.0), True, hankel_eps=1e-9)
    assert td["hankel_eps"] == 1e-9 and "hankel_eps_ppm" not in td and td["solve_receiver_pitch"] is True and td["maximum_receiver_pitch_change"] == 5.0
    assert "solve_receiver_pitch" not in survey_run.sampler_arguments(dict(o, solve_receiver_pitch=True), False)
    assert not {"hankel_eps", "hankel_eps_ppm"} & set(kw)
    # unit and threshold arguments; data posteriors
    assert not {"first_above", "first_below", "unit_kinds", "data_posteriors"} & set(kw)
    un = survey_run.sampler_arguments(o, False, units=True, unit_kinds=("harmonic",), first_below=[0.01])
    assert un["unit_kinds"] == ("harmonic",) and un["first_above"] == () and un["first_below"] == (0.01,)
    with pytest.raises(ValueError, match="need the hit map"):
        survey_run.sampler_arguments(o, False, hitmap=False, first_above=(0.1,))
    dp = survey_run.sampler_arguments(o, False, data_posteriors=dict(n_bins=32))
    assert dp["data_posteriors"] == dict(n_bins=32, half_width=8.0, misfit_half_width=2.0)
    assert survey_run.sampler_arguments(o, False, data_posteriors=True)["data_posteriors"]["n_bins"] == 64
    assert "data_posteriors" not in survey_run.sampler_arguments(o, False, data_posteriors=False)
    with pytest.raises(ValueError, match="takes no scale"):
        survey_run.sampler_arguments(o, False, data_posteriors=dict(scale=np.ones(12)))
    with pytest.raises(ValueError, match="need the hit map"):
        survey_run.sampler_arguments(o, False, hitmap=False, data_posteriors=True)


def test_request_checks_keep_their_refusals():
    o = survey.read_options(OPTIONS)
    assert survey_run.check_request(o, True, 1) == (False, False, 1) and survey_run.check_request(o, True, "4") == (False, False, 4)
    assert survey_run.check_request(dict(o, data_type="TempestData"), True, 1) == (True, True, 1)
    for bad, kind, text in ((dict(o, data_type="Other"), NotImplementedError, "Other is not supported"),
                            (dict(o, solve_receiver_pitch=True), NotImplementedError, "solve_receiver_pitch: frequency-domain"),
                            (dict(o, solve_calibration=True), NotImplementedError, "solve_calibration"),
                            (dict(o, data_type="TdemData", ignore_likelihood=True), NotImplementedError, "prior-only"),
                            (dict(o, data_type="TdemData", solve_z=True), NotImplementedError, "TRANSMITTER")):
        with pytest.raises(kind, match=text):
            survey_run.check_request(bad, True, 1)
    with pytest.raises(ValueError, match="1 .. 8"):
        survey_run.check_request(o, True, 9)
    with pytest.raises(NotImplementedError, match="replicates > 1 on time-domain"):
        survey_run.check_request(dict(o, data_type="TdemData"), True, 2)
    with pytest.raises(ValueError, match="needs the hit map"):
        survey_run.check_request(o, False, 2)


def _stand_in_sampler(**kw):
    d = dict(N=4, K=3, n_depth_bins=5, n_value_bins=2, n_rel_groups=1, n_add_groups=2)
    d.update(kw)
    return SimpleNamespace(**d)


def test_device_rows_are_packed_in_the_order_the_writer_reads():
    """pack_rows puts {field: tensor} in the order of hdf.device_row_fields, asked through the one helper _LineWriter asks through
    (survey._row_fields): every field at the offset the writer slices it at, whatever the order the dict was built in; a field that is
    not there, or has another width, is an error that names it."""
    ds = SimpleNamespace()                                      # (not a TdemData: frequency-domain rows)
    dc = _stand_in_sampler(solve_height=True, trace_length=6)
    ff, fi, fkw = survey._row_fields(ds, dc, True)
    assert (ff, fi) == hdf.device_row_fields(4, 3, 5, 2, **fkw) and fkw == dict(hitmap=True, n_rel=1, n_add=2, time_domain=False, n_primary=0,
                                                                                height=True, angles=(), trace_length=6)
    assert [n for n, _ in ff][-3:] == ["best_height", "height0", "trace_misfit"] and [n for n, _ in fi][-3:] == ["hitmap", "height_hist", "trace_accept"]
    for layout, dtype in ((ff, None), (fi, torch.int32)):
        fields = {n: torch.full((3, w), float(j), dtype=torch.float64 if dtype is None else torch.int64) for j, (n, w) in enumerate(layout)}
        shuffled = dict(reversed(list(fields.items())), not_a_field=torch.zeros(3, 1))
        block = survey_run.pack_rows(shuffled, layout, dtype)
        assert block.shape == (3, sum(w for _, w in layout)) and block.dtype == (torch.float64 if dtype is None else torch.int32) and block.is_contiguous()
        c = 0
        for j, (n, w) in enumerate(layout):
            assert torch.all(block[:, c:c + w] == j), n
            c += w
        name = layout[4][0]
        with pytest.raises(KeyError, match=name):
            survey_run.pack_rows({k: v for k, v in fields.items() if k != name}, layout, dtype)
        with pytest.raises(ValueError, match="'{}'".format(name)):
            survey_run.pack_rows(dict(fields, **{name: torch.zeros(3, layout[4][1] + 1)}), layout, dtype)
        with pytest.raises(ValueError, match="'{}'".format(name)):
            survey_run.pack_rows(dict(fields, **{name: torch.zeros(3)}), layout, dtype)
    # without the hit map's columns (it travels as runs), without height and traces: the same helper, fewer fields
    _, fi0, _ = survey._row_fields(ds, _stand_in_sampler(), False)
    assert [n for n, _ in fi0] == ["status", "burned_in_iteration", "iterations", "best_k", "best_iteration", "k_hist", "edge_hist", "rel_hist", "add_hist"]
    # a field of width 0 (a time-domain system without primary-field columns) has no column and need not be there
    assert survey_run.pack_rows(dict(a=torch.ones(2, 1), c=torch.zeros(2, 2)), [("a", 1), ("b", 0), ("c", 2)]).tolist() == [[1.0, 0.0, 0.0]] * 2


class _Writer:
    def __init__(self, fail_on=None):
        self.blocks, self.finished, self.fail_on = [], 0, fail_on

    def add_block(self, block):
        if block == self.fail_on:
            raise RuntimeError("writer refused block {}".format(block))
        self.blocks.append((block, threading.current_thread() is threading.main_thread()))

    def finish(self):
        self.finished += 1
        return ["paths"]


class _Blocks:
    """A payload function that counts the fills in flight and lets the test hold one back."""

    def __init__(self):
        self.in_flight, self.most, self.gate, self.lock = 0, 0, threading.Event(), threading.Lock()
        self.gate.set()

    def __call__(self, dc, idx):
        with self.lock:
            self.in_flight += 1
            self.most = max(self.most, self.in_flight)
        assert self.gate.wait(10.0)
        with self.lock:
            self.in_flight -= 1
        return dc.name


def _filler(payload, writer, timings=None):
    made = []
    filler = survey_run.ContainerFiller(payload, lambda dc: made.append(dc.name) or writer, survey_run.PhaseClock(timings), device_stream=False)
    return filler, made


def test_filler_hands_the_blocks_over_in_order_one_at_a_time():
    payload, writer, timings = _Blocks(), _Writer(), {}
    filler, made = _filler(payload, writer, timings)
    block = lambda name, n=2: (SimpleNamespace(name=name), np.arange(n))
    with filler:
        filler.drain(background=True)                             # (nothing handed over yet: nothing happens)
        assert filler.writer is None and filler.thread is None
        payload.gate.clear()                                      # a's fill is held back ...
        filler.hand_over(*block("a"))
        filler.drain(background=True)                             # ... and runs beside the caller ("the next block's chains")
        assert filler.unfilled is None and filler.thread.is_alive() and payload.in_flight <= 1 and writer.blocks == []
        filler.hand_over(*block("b"))
        release = threading.Timer(0.05, payload.gate.set)
        release.start()
        filler.drain(background=True)                             # waits for a before it starts b
        assert writer.blocks[0] == ("a", False) and filler.thread is not None
        filler.hand_over(*block("c"))
        filler.drain(background=True)
        assert [b for b, _ in writer.blocks][:2] == ["a", "b"]
        release.join()
    assert filler.thread is None and [b for b, _ in writer.blocks] == ["a", "b", "c"] and payload.most == 1 and made == ["a"]
    assert not any(main for _, main in writer.blocks)             # all three on the fill thread
    assert set(timings) == {"rows_to_host_overlapped", "container_fill_overlapped"}
    # the last block goes in the foreground, then the writer ends; an empty block makes the writer and hands nothing over
    filler.hand_over(*block("d"))
    assert filler.finish(SimpleNamespace(name="unused")) == ["paths"] and writer.blocks[-1] == ("d", True) and writer.finished == 1 and made == ["a"]
    assert set(timings) == set(survey_run.PHASES) & set(timings) and {"rows_to_host", "container_fill", "compress_and_write_tail"} <= set(timings)
    empty, made = _filler(payload, _Writer())
    empty.hand_over(*block("e", 0))
    empty.drain(background=True)
    assert made == ["e"] and empty.thread is None and empty.writer.blocks == []
    none, made = _filler(payload, _Writer())                      # no sounding at all: the empty set of containers
    assert none.finish(SimpleNamespace(name="last")) == ["paths"] and made == ["last"]
    # timings=None: the clock does nothing
    quiet, _ = _filler(payload, _Writer())
    quiet.hand_over(*block("f"))
    quiet.drain(background=True)
    quiet.finish(None)
    assert quiet.clock.timings is None and [b for b, _ in quiet.writer.blocks] == ["f"]


def test_filler_reports_a_failed_fill_in_the_callers_thread():
    block = lambda name: (SimpleNamespace(name=name), np.arange(2))
    # ... at the next drain
    filler, _ = _filler(_Blocks(), _Writer(fail_on="a"))
    with pytest.raises(RuntimeError, match="refused block a"):
        with filler:
            filler.hand_over(*block("a"))
            filler.drain(background=True)
            filler.hand_over(*block("b"))
            filler.drain(background=True)
            raise AssertionError("the second drain must raise what the fill of a raised")
    assert filler.thread is None and filler.failed == [] and filler.writer.blocks == []
    # ... or at the exit, when the body has nothing more to drain
    filler, _ = _filler(_Blocks(), _Writer(fail_on="a"))
    with pytest.raises(RuntimeError, match="refused block a"):
        with filler:
            filler.hand_over(*block("a"))
            filler.drain(background=True)
    assert filler.thread is None and filler.failed == []


def test_filler_joins_its_thread_when_the_caller_raises():
    block = lambda name: (SimpleNamespace(name=name), np.arange(2))
    payload, writer = _Blocks(), _Writer()
    filler, _ = _filler(payload, writer)
    payload.gate.clear()
    release = threading.Timer(0.05, payload.gate.set)             # the fill is still running when the caller raises
    before = threading.active_count()
    with pytest.raises(KeyError, match="the caller's own") as seen:
        with filler:
            filler.hand_over(*block("a"))
            filler.drain(background=True)
            th = filler.thread
            release.start()
            raise KeyError("the caller's own")
    release.join()
    assert not th.is_alive() and filler.thread is None and threading.active_count() == before
    assert [b for b, _ in writer.blocks] == ["a"] and seen.value.__context__ is None
    # both fail: the caller's exception is the one seen, the fill's is attached to it
    filler, _ = _filler(_Blocks(), _Writer(fail_on="a"))
    with pytest.raises(KeyError, match="the caller's own") as seen:
        with filler:
            filler.hand_over(*block("a"))
            filler.drain(background=True)
            raise KeyError("the caller's own")
    assert isinstance(seen.value.__context__, RuntimeError) and "refused block a" in str(seen.value.__context__)
    assert filler.thread is None and filler.failed == []


def test_phase_clock_accumulates_only_when_asked():
    clock = survey_run.PhaseClock(None)
    with clock.phase("chains"):
        pass
    clock.add("chains", 1.0)
    assert clock.timings is None
    t = {}
    clock = survey_run.PhaseClock(t)
    for _ in range(2):
        with clock.phase("chains"):
            pass
    clock.add("rows_to_host_overlapped", 0.25)
    clock.add("rows_to_host_overlapped", 0.5)
    with pytest.raises(ZeroDivisionError):
        with clock.phase("container_fill"):
            1 / 0
    assert set(t) == {"chains", "rows_to_host_overlapped", "container_fill"} and t["rows_to_host_overlapped"] == 0.75 and t["chains"] >= 0.0


def _entries(rows):
    """Hand-made summaries: tails (), (1,) squeezed, (1,) kept, (3,), (2, 5) and (0,); results int32, int64, bool and float64 from
    tensors of their own or of another dtype; NaN and the largest int32 among the values -> ([Entry], {name: the expected array})."""
    E, big = survey_run.Entry, 2 ** 31 - 1
    count = torch.arange(rows, dtype=torch.int32) * 3 - 1
    if rows:
        count[0] = big
    real = torch.arange(rows * 10, dtype=torch.float64).reshape(rows, 2, 5) / 7.0
    real[:1, 1, 2] = float("nan")
    flag = (torch.arange(rows * 3).reshape(rows, 3) % 2) == 0
    entries = [E("scalar", count), E("squeezed", real[:, 1, 2:3]), E("kept", real[:, :1, 0], keep=True), E("kept_count", count[:, None], np.int64, True),
               E("flags", flag), E("cube", real), E("single", real[:, 0, :3].to(torch.float32)), E("nothing", real[:, 0, :0]),
               E("wide_count", count[:, None].to(torch.int64) + torch.arange(2), np.float64), E("bytes", flag.to(torch.uint8), np.int32)]
    expected = dict(scalar=count.numpy(), squeezed=real[:, 1, 2].numpy(), kept=real[:, :1, 0].numpy(), kept_count=count[:, None].numpy().astype(np.int64),
                    flags=flag.numpy(), cube=real.numpy(), single=real[:, 0, :3].to(torch.float32).numpy().astype(np.float64), nothing=np.zeros((rows, 0)),
                    wide_count=(count[:, None].to(torch.int64) + torch.arange(2)).numpy().astype(np.float64), bytes=flag.numpy().astype(np.int32))
    return entries, expected


@pytest.mark.parametrize("rows", [0, 4])
def test_result_rows_pack_and_unpack_exactly(rows):
    entries, expected = _entries(rows)
    columns = survey_run.layout(entries)
    assert [(name, tail, dtype.name, squeeze) for name, tail, dtype, squeeze in columns] == [
        ("scalar", (), "int32", True), ("squeezed", (1,), "float64", True), ("kept", (1,), "float64", False), ("kept_count", (1,), "int64", False),
        ("flags", (3,), "bool", True), ("cube", (2, 5), "float64", True), ("single", (3,), "float64", True), ("nothing", (0,), "float64", True),
        ("wide_count", (2,), "float64", True), ("bytes", (3,), "int32", True)]
    assert columns == survey_run.layout(_entries(4 - rows)[0])          # an empty block gives the layout of a full one
    block = survey_run.pack(entries)
    assert block.dtype == torch.float64 and block.shape == (rows, 1 + 1 + 1 + 1 + 3 + 10 + 3 + 0 + 2 + 3) and block.is_contiguous()
    got = survey_run.unpack(columns, block.numpy())
    assert list(got) == [e.name for e in entries]
    for name, want in expected.items():
        assert got[name].dtype == want.dtype and got[name].shape == want.shape and np.array_equal(got[name], want, equal_nan=want.dtype.kind == "f"), name
    assert rows == 0 or (got["scalar"][0] == 2 ** 31 - 1 and np.isnan(got["squeezed"][0]) and np.isnan(got["cube"][0, 1, 2]))


def test_the_column_order_belongs_to_the_layout():
    entries, expected = _entries(4)
    a, b = [entries[5], entries[0], entries[4]], [entries[4], entries[5], entries[0]]
    la, lb = survey_run.layout(a), survey_run.layout(b)
    assert [c[0] for c in la] == ["cube", "scalar", "flags"] and [c[0] for c in lb] == ["flags", "cube", "scalar"] and set(la) == set(lb)
    pa, pb = survey_run.pack(a).numpy(), survey_run.pack(b).numpy()
    assert pa.shape == pb.shape and np.array_equal(pa[:, 10], expected["scalar"]) and np.array_equal(pb[:, 13], expected["scalar"])
    for lay, block in ((la, pa), (lb, pb)):
        got = survey_run.unpack(lay, block)
        assert list(got) == [c[0] for c in lay] and all(np.array_equal(got[k], expected[k], equal_nan=k == "cube") for k in got)
    assert not np.array_equal(survey_run.unpack(lb, pa)["flags"], expected["flags"])        # rows of one order read with the other's layout


def test_assemble_result_keeps_the_dtypes():
    ds = SimpleNamespace(lineNumber=np.zeros(3), fiducial=np.arange(3.0), x=np.zeros(3), y=np.zeros(3), z=np.zeros(3), elevation=np.zeros(3))
    dc = SimpleNamespace(depth_bin_width=0.5)
    i32, i64, f64 = np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.float64)
    columns = [(k, tail, dtype, True) for k, tail, dtype in (
        ("status", (), i32), ("burned_in_iteration", (), i32), ("n_accepted", (), i64), ("misfit", (), f64), ("relative_error", (1,), f64),
        ("additive_error", (2,), f64), ("n_layers", (), i32), ("best_n_layers", (), i32), ("layer_count_posterior", (3,), i64),
        ("additive_error_posterior", (2, 2), i64), ("mean_log10_conductivity", (4,), f64))]
    r = np.zeros((3, 20))
    r[:, 0], r[:, 1], r[:, 2] = [1, 2, 0], [10, 0, 0], [50, 20, 30]
    res = survey_run.assemble_result(ds, {"n_markov_chains": 100}, dc, columns, r, 77)
    assert res["iterations"].tolist() == [111, 100, 77] and res["iterations"].dtype == np.int64 and "n_accepted" not in res
    assert np.array_equal(res["acceptance"], [50 / 111, 0.2, 30 / 77])
    for k in ("status", "burned_in_iteration", "n_layers", "best_n_layers"):
        assert res[k].dtype == np.int32 and res[k].shape == (3,)
    assert res["layer_count_posterior"].dtype == np.int64 and res["additive_error_posterior"].shape == (3, 2, 2) and res["additive_error_posterior"].dtype == np.int64
    assert res["misfit"].dtype == np.float64 and res["mean_log10_conductivity"].shape == (3, 4) and res["depth_bin_width"] == 0.5


def test_summaries_declare_what_the_result_holds():
    """SurveyRun.summaries itself, on a stand-in sampler of host tensors (no hit map, so no kernel runs): sampled height and one sampled
    angle, two error groups, two replicate chains -- the counts come back int32, the posteriors' counts and the replicates' counts
    int64, through layout, pack and unpack."""
    S, C, nd, K = 3, 2, 4, 3
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt)
    i32 = torch.int32
    t = dict(status=z(S, dt=i32), burned_in_iteration=z(S, dt=i32), n_accepted=z(S, dt=torch.int64), misfit=z(S), rel=z(S, 1), add=z(S, 2),
             k=z(S, dt=i32), best_k=z(S, dt=i32), best_posterior=z(S), best_edges=z(S, K), best_sigma=z(S, K), k_hist=z(S, K + 1, dt=i32),
             edge_hist=z(S, nd, dt=i32), rel_hist=z(S, 1, 99, dt=i32), add_hist=z(S, 2, 99, dt=i32), geom_hist=z(S, 1, 199, dt=i32),
             height=z(S), best_height=z(S), height_hist=z(S, 99, dt=i32))
    dc = SimpleNamespace(t=t, _moves=[("rx_pitch", None, None, None, None, 7)], sampled_angles=lambda which: {"rx_pitch": z(S)},
                         solve_height=True, use=torch.ones(S, C, dtype=torch.bool))
    diag = dict(rhat=z(S, nd), jsd=z(S, nd), n_used=z(S, nd, dt=i32), chain_mean=z(S, C, nd), rhat_layers=z(S), jsd_layers=z(S),
                rhat_interfaces=z(S), rhat_max=z(S))
    run = SimpleNamespace(clock=survey_run.PhaseClock(None), hitmap=False, C_rep=C, ensemble_diagnostics=None, ensemble_correlation=None,
                          ensemble_families=None)
    entries = survey_run.SurveyRun.summaries(run, dc, diag)
    res = survey_run.unpack(survey_run.layout(entries), survey_run.pack(entries).numpy())
    assert list(res)[-len(survey.REPLICATE_SUMMARIES) - 1:] == list(survey.REPLICATE_SUMMARIES) + ["replicates_used"]
    for k in ("status", "burned_in_iteration", "n_layers", "best_n_layers"):
        assert res[k].dtype == np.int32 and res[k].shape == (S,)
    for k, shape in (("n_used", (S, nd)), ("replicates_used", (S,)), ("rx_pitch_posterior", (S, 7)), ("height_posterior", (S, 99)),
                     ("layer_count_posterior", (S, K + 1)), ("interface_posterior", (S, nd)), ("relative_error_posterior", (S, 99)),
                     ("additive_error_posterior", (S, 2, 99))):
        assert res[k].dtype == np.int64 and res[k].shape == shape, k
    assert res["replicates_used"].tolist() == [C] * S
    for k, shape in (("relative_error", (S,)), ("additive_error", (S, 2)), ("rx_pitch", (S,)), ("best_height", (S,)), ("chain_mean", (S, C, nd)),
                     ("rhat", (S, nd)), ("rhat_max", (S,)), ("best_edges", (S, K))):
        assert res[k].dtype == np.float64 and res[k].shape == shape, k
