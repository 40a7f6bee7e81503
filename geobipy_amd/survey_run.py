"""The parts of a survey run, in the order ``survey.infer`` uses them: the request's checks and the sampler's arguments, the block size
and the schedule, the run itself (one block's chains, its summaries, its device rows), the phase clock, the container filler and the
assembly of the result.  ``survey.infer`` imports this module when it is called; nothing here is needed to read options or data."""
import contextlib
import math
import threading
import time
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np
import torch

from .survey import (BLOCK_PAYLOAD_BUDGET, REPLICATE_SUMMARIES, SurveyResult, TdemData, TempestData, _hitmap_statistics,
                     _row_fields, _write_line_containers)

# the phase clock's names (bench.py reads them from survey.infer(timings={}))
PHASES = ("upload_and_initialise", "chains", "pool_replicates", "hitmap_statistics", "unit_posteriors", "data_posteriors", "ensemble", "rows_to_host",
          "container_fill", "rows_to_host_overlapped", "container_fill_overlapped", "compress_and_write_tail", "summaries_to_host",
          "summary_file_tail")

# the options the samplers take under their own names
OPTION_KEYS = ("ignore_likelihood", "n_markov_chains", "solve_gradient", "solve_parameter", "solve_relative_error", "solve_additive_error",
               "maximum_number_of_layers", "minimum_depth", "maximum_depth", "minimum_thickness", "initial_relative_error",
               "minimum_relative_error", "maximum_relative_error", "initial_additive_error", "minimum_additive_error",
               "maximum_additive_error", "relative_error_proposal_variance", "additive_error_proposal_variance", "probability_of_birth",
               "probability_of_death", "probability_of_perturb", "probability_of_no_change", "factor", "gradient_standard_deviation",
               "covariance_scaling", "parameter_limits", "update_plot_every", "reset_limit", "solve_z", "maximum_z_change",
               "z_proposal_variance")


# ---- the request --------------------------------------------------------------------------------------------------------------------

def check_request(o, hitmap, replicates):
    """What the device sampler refuses of an options dict -> (tempest, time_domain, replicate chains per sounding)."""
    tempest = o["data_type"] in ("TempestData", "Tempest_datapoint")
    time_domain = tempest or o["data_type"] in ("TdemData", "TdemDataPoint")
    if not time_domain and o["data_type"] not in ("FdemData", "FdemDataPoint"):
        raise NotImplementedError("the device sampler handles FdemData, TdemData and TempestData; {} is not supported".format(o["data_type"]))
    geometry_keys = [k_ for k_ in o if (k_.startswith("solve_transmitter_") or k_.startswith("solve_receiver_")) and o[k_]]
    if geometry_keys and not time_domain:
        raise NotImplementedError(geometry_keys[0] + ": frequency-domain data points have no loop pair to sample")
    # (time-domain data: the loops' attitude angles are sampled on the device, gbp_td_moves; position moves raise in TdemDeviceChains)
    if o.get("solve_calibration"):
        raise NotImplementedError("solve_calibration is not supported by the device sampler")
    if o.get("ignore_likelihood") and time_domain:
        raise NotImplementedError("ignore_likelihood (prior-only sampling) on time-domain data is not supported by the device sampler")
    # (frequency-domain data: DeviceChains(ignore_likelihood=True) -- the prior alone, Inference1D.py:394, 519, 551, 596)
    # solve_height: the reference's datapoint only moves its height for the keys solve_z / maximum_z_change /
    # z_proposal_variance (pointcloud/Point.py:949-983), which its options files never set -- with the files as shipped the height
    # stays fixed there too.  An options file that DOES carry solve_z = True gets the move (frequency-domain data; DeviceChains).
    if time_domain and o.get("solve_z"):
        raise NotImplementedError("solve_z on time-domain data: the reference's forward takes the TRANSMITTER's z (system/Loop_pair.py:70), "
                                  "which the data point's z move never touches -- the key that would matter is solve_transmitter_z, and the "
                                  "geometry of the loop pair is not sampled")
    C_rep = int(replicates)
    if not 1 <= C_rep <= 8:
        raise ValueError("replicates = {}: 1 .. 8 chains per sounding".format(replicates))
    if C_rep > 1 and time_domain:
        raise NotImplementedError("replicates > 1 on time-domain data: the system handle holds per-row state (table set, mixing weights), "
                                  "which the pooled view would have to re-map for the best-model evaluation")
    if C_rep > 1 and not hitmap:
        raise ValueError("replicates > 1 needs the hit map (the convergence maps are computed from the chains' hit maps)")
    return tempest, time_domain, C_rep


def sampler_arguments(o, time_domain, seed=None, device=None, hitmap=True, first_chain=0, burn_in_min_iterations=5000, containers=False,
                      traces=1, units=False, unit_kinds=("arithmetic", "harmonic"), first_above=(), first_below=(), data_posteriors=None,
                      hankel_eps=None, ensemble=None):
    """The keyword arguments every block's DeviceChains / TdemDeviceChains gets, from the options ``o`` and infer's own arguments
    (``containers``: results containers are written; ``units``: a unit spec was given -- its bounds are per block, SurveyRun.unit_z).
    Touches no device."""
    keys = OPTION_KEYS
    if time_domain:
        from .tdem_geometry import LOOP_PAIR_SCALARS
        keys = keys + tuple(k_ for _, stem, _ in LOOP_PAIR_SCALARS for k_ in ("solve_" + stem, "maximum_" + stem + "_change", stem + "_proposal_variance"))
    seed = o.get("seed", 0) if seed is None else seed
    common = dict(seed=int(seed) % (1 << 64), device=device, hitmap=hitmap, first_chain=int(first_chain), reference_schedule=True,
                  burn_in_min_iterations=burn_in_min_iterations, **{k: o[k] for k in keys if o.get(k) is not None})
    # per-iteration traces for the containers' `phids` / `acceptance_rate` (Inference1D.data_misfit_v / acceptance_v): kept on the
    # device at a stride -- "auto": the smallest stride with at most 4 096 entries per sounding (32 + 4 KB per sounding beside a
    # 440 KB hit map; the reference's full arrays are 2 n_markov_chains x 9 bytes = 1.8 MB at its default 100 000); an int: that
    # stride (1 = the reference's arrays in full); None / 0: no traces (the two datasets stay at their fill values)
    if containers and traces:
        n_mc2 = 2 * int(o["n_markov_chains"])
        common.update(trace_every=max(1, -(-n_mc2 // 4096)) if traces == "auto" else int(traces))
    if units or len(first_above) or len(first_below):
        if not hitmap:
            raise ValueError("units / first_above / first_below need the hit map (they are settled with its dwell times)")
        common.update(first_above=tuple(float(v) for v in first_above), first_below=tuple(float(v) for v in first_below), unit_kinds=unit_kinds)
    if data_posteriors is not None and data_posteriors is not False:
        from .inference import data_posteriors_argument
        dp = data_posteriors_argument(data_posteriors)
        if not hitmap:
            raise ValueError("data_posteriors need the hit map (they are settled with its dwell times)")
        if dp["scale"] is not None:
            raise ValueError("data_posteriors: survey.infer takes no scale (each channel's standard deviation at the initial error levels)")
        common.update(data_posteriors={k_: dp[k_] for k_ in ("n_bins", "half_width", "misfit_half_width")})
    if ensemble is not None and ensemble is not False:
        from .inference import ensemble_argument
        if not hitmap:
            raise ValueError("ensemble needs the hit map (it is settled with its dwell times)")
        common.update(ensemble=ensemble_argument(ensemble, n_markov_chains=o.get("n_markov_chains"), reference_schedule=True))
    if hankel_eps is not None:
        common.update({"hankel_eps" if time_domain else "hankel_eps_ppm": float(hankel_eps)})
    return common


def _ensemble_product_argument(name, keys, value, ensemble, needs):
    """What infer's ``ensemble_*`` arguments share: False / None -> None (off); True -> {}; a dict of ``keys`` -> that dict.  Anything
    else is refused, and so is any of them without ``ensemble`` (``needs``: why the product needs it)."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict) or set(value) - set(keys):
        raise ValueError("{}: False, True or dict({})".format(name, ", ".join(k_ + "=" for k_ in keys)))
    if ensemble is None or ensemble is False:
        raise ValueError("{} needs ensemble= ({})".format(name, needs))
    return value


def ensemble_diagnostics_argument(ensemble_diagnostics, ensemble):
    """infer's ``ensemble_diagnostics`` (False / None: off; True; dict(max_lag=)) as None or dict(max_lag=int in 1 .. 255).  Refuses
    the diagnostics without an ensemble.  Touches no device."""
    given = _ensemble_product_argument("ensemble_diagnostics", ("max_lag",), ensemble_diagnostics, ensemble, "the diagnostics are computed from the kept models")
    if given is None:
        return None
    from .ensembles import check_max_lag
    return dict(max_lag=check_max_lag(given.get("max_lag")))


def ensemble_rank_diagnostics_argument(ensemble_rank_diagnostics, ensemble):
    """infer's ``ensemble_rank_diagnostics`` (False / None: off; True; dict(max_lag=, percentiles=)) as None or dict(max_lag=int in
    1 .. 255, percentiles=ascending floats in [0, 100]).  Refuses the rank diagnostics without an ensemble.  Touches no device."""
    given = _ensemble_product_argument("ensemble_rank_diagnostics", ("max_lag", "percentiles"), ensemble_rank_diagnostics, ensemble,
                                       "the ranks are those of the kept models")
    if given is None:
        return None
    from .ensembles import check_max_lag, check_percentiles
    return dict(max_lag=check_max_lag(given.get("max_lag")), percentiles=check_percentiles(given.get("percentiles", (5, 50, 95))))


def ensemble_correlation_argument(ensemble_correlation, ensemble):
    """infer's ``ensemble_correlation`` (False / None: off; True; dict(band=, threshold=, keep_band=)) as None or dict(band=int >= 0,
    threshold=float in (0, 1), keep_band=bool).  Refuses the correlation without an ensemble.  Touches no device."""
    ensemble_correlation = _ensemble_product_argument("ensemble_correlation", ("band", "threshold", "keep_band"), ensemble_correlation, ensemble,
                                                      "the correlation is computed from the kept models")
    if ensemble_correlation is None:
        return None
    from .ensembles import check_threshold
    band = ensemble_correlation.get("band", 64)
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or int(band) < 0:
        raise ValueError("ensemble_correlation: band must be an integer >= 0")
    keep = ensemble_correlation.get("keep_band", False)
    if not isinstance(keep, (bool, np.bool_)):
        raise ValueError("ensemble_correlation: keep_band is True or False")
    return dict(band=int(band), threshold=check_threshold(ensemble_correlation.get("threshold", 0.5)), keep_band=bool(keep))


def ensemble_families_argument(ensemble_families, ensemble):
    """infer's ``ensemble_families`` (False / None: off; True; dict(max_families=, max_models=, measure=, min_silhouette=)) as None or
    dict(max_families=int in 1 .. 8, max_models=int in 1 .. 4096, measure="linear" | "log", min_silhouette=float in [0, 1]).  Refuses
    before any device work."""
    ensemble_families = _ensemble_product_argument("ensemble_families", ("max_families", "max_models", "measure", "min_silhouette"),
                                                   ensemble_families, ensemble, "the families are made of the kept models")
    if ensemble_families is None:
        return None
    from .families import MAX_FAMILIES, MAX_MODELS, MEASURES
    out = dict(max_families=ensemble_families.get("max_families", 4), max_models=ensemble_families.get("max_models", 1024),
               measure=ensemble_families.get("measure", "linear"), min_silhouette=ensemble_families.get("min_silhouette", 0.7))
    for name, hi in (("max_families", MAX_FAMILIES), ("max_models", MAX_MODELS)):
        v = out[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
            raise ValueError("ensemble_families: %s must be an integer in 1 .. %d" % (name, hi))
        out[name] = int(v)
    if out["measure"] not in MEASURES:
        raise ValueError("ensemble_families: measure must be 'linear' or 'log'")
    if out["measure"] == "log":
        raise ValueError("ensemble_families: the window starts at the surface (z0 = 0), which the log measure cannot weigh; use families.families")
    v = out["min_silhouette"]
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError("ensemble_families: min_silhouette must be a number in [0, 1]")
    out["min_silhouette"] = float(v)
    return out


def ensemble_bytes(n_keep, max_layers):
    """Bytes of device memory one chain's posterior ensemble takes: n_keep slots of 2 K doubles, a misfit and a layer count, and the
    chain's sample counter -- n_keep (16 K + 12) + 4 (126 KB at n_keep = 256, K = 30, beside the hit map's 440 KB)."""
    return int(n_keep) * (16 * int(max_layers) + 12) + 4


# ---- block size and schedule --------------------------------------------------------------------------------------------------------

def default_block(n_markov_chains, trace_every, payload_hitmap, replicates, limit=16384, ensemble_bytes=0):
    """Default block size: ``limit`` soundings, less when a sounding's posterior payload on the device is large -- full-length traces at
    the reference's default n_markov_chains = 100 000 are 1.8 MB per sounding (29.5 GB for 16 384, plus their host copies): the default
    block keeps traces + hit maps under BLOCK_PAYLOAD_BUDGET.  Chains are keyed by row, so the block size never changes a result.
    ``trace_every``: the traces' stride (None / 0: none kept); ``payload_hitmap``: the hit maps leave the device for the containers;
    ``ensemble_bytes``: a chain's posterior ensemble (``ensemble_bytes()``; 0: none kept), counted in the same budget."""
    per = int(ensemble_bytes)
    if trace_every:
        per += -(-2 * int(n_markov_chains) // int(trace_every)) * 9        # misfit f64 + acceptance u8 per kept entry
    if payload_hitmap:
        per += 440 * 1024                                                   # (the hit map's usual size; exact: DeviceChains)
    if replicates > 1:                              # a sounding is C rows of the block
        limit, per = max(1, limit // replicates), per * replicates
    return limit if per == 0 else int(max(256 // replicates, min(limit, BLOCK_PAYLOAD_BUDGET // per)))


def line_runs(line_numbers):
    """The runs of consecutive rows with one line number -> (first row of every run, rows per run, every flight line is ONE run)."""
    line_numbers = np.asarray(line_numbers)
    if line_numbers.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), True
    firsts = np.r_[0, np.flatnonzero(np.diff(line_numbers) != 0) + 1]
    return firsts, np.diff(np.r_[firsts, line_numbers.size]), bool(np.unique(line_numbers[firsts]).size == firsts.size)


def auto_schedule(line_numbers, world, containers):
    """schedule="auto".  More than one rank: whole lines per rank ("lines") -- every rank writes its own containers and the job's only
    exchange is the gather of the one-row summaries (all_gather_into_tensor; the posterior rows of "static" / "dynamic" travel point
    to point, which has run over gloo only) -- whenever the data file allows it (every flight line one run of consecutive rows) and
    whole lines balance: the most loaded rank within 1.2 x the mean (a survey with fewer lines than ranks, or one dominant line, would
    leave GPUs idle where "static" uses all of them); without containers "lines" buys nothing.  Else "static"."""
    from .distributed import assign_lines
    firsts, counts, one_run_per_line = line_runs(line_numbers)
    if not (world > 1 and containers and firsts.size and one_run_per_line and firsts.size >= world):
        return "static"
    loads = [int(sum(counts[i] for i in mine)) for mine in assign_lines(counts, world)]
    return "lines" if max(loads) <= 1.2 * counts.sum() / world else "static"


# ---- the phase clock ----------------------------------------------------------------------------------------------------------------

class PhaseClock:
    """Wall time by phase into the caller's dict ``timings``, device-synchronised at the phase borders; with ``timings`` None (a normal
    run) it does nothing and never synchronises for this."""

    def __init__(self, timings):
        self.timings = timings

    def add(self, name, seconds):
        if self.timings is not None:
            self.timings[name] = self.timings.get(name, 0.0) + seconds

    def _border(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return time.perf_counter()

    @contextlib.contextmanager
    def phase(self, name):
        if self.timings is None:
            yield
            return
        t0 = self._border()
        try:
            yield
        finally:
            self.add(name, self._border() - t0)


# ---- the device rows of a block -----------------------------------------------------------------------------------------------------

def pack_rows(fields, layout, dtype=None):
    """One [rows, sum of widths] block from ``fields`` {name: [rows, width] tensor} in the order of ``layout`` [(name, width)] (one of
    the two lists of hdf.device_row_fields; a field of width 0 has no column and need not be there).  A field the layout names and
    ``fields`` lacks is a KeyError, one of another width a ValueError."""
    cols = []
    for name, w in layout:
        if w == 0:
            continue
        v = fields[name]
        if v.ndim != 2 or v.shape[1] != w:
            raise ValueError("device rows: field '{}' has shape {}, the layout gives it {} column(s)".format(name, tuple(v.shape), w))
        cols.append(v if dtype is None else v.to(dtype))
    return torch.cat(cols, dim=1).contiguous()


# ---- the result rows of a block -----------------------------------------------------------------------------------------------------

class Entry(NamedTuple):
    """One per-sounding summary as ``SurveyRun.summaries`` holds it."""
    name: str
    tensor: object                      # [rows, ...], in the shape and dtype it has on the device
    dtype: object = None                # the result's numpy dtype, where it is not the tensor's own (a floating tensor's: float64)
    keep: bool = False                  # a single column stays [rows, 1] (default: it comes back [rows])


def layout(entries):
    """[(name, tail, dtype, squeeze)] of ``entries``, in their order: the result's shape after the soundings' axis, its numpy dtype, and
    whether a single column comes back [rows].  Rows are not looked at, so an empty block gives the layout of a full one."""
    own = lambda v: np.float64 if v.is_floating_point() else torch.empty(0, dtype=v.dtype).numpy().dtype      # noqa: E731
    return tuple((e.name, tuple(e.tensor.shape[1:]), np.dtype(own(e.tensor) if e.dtype is None else e.dtype), not e.keep) for e in entries)


def pack(entries):
    """The float64 [rows, sum of widths] block of ``entries``, the columns in their order: what the ranks exchange (counts are 32-bit
    on the device and flags 0 / 1, so float64 holds them exactly)."""
    return torch.cat([e.tensor.to(torch.float64).reshape(e.tensor.shape[0], math.prod(e.tensor.shape[1:])) for e in entries], dim=1).contiguous()


def unpack(columns, block):
    """{name: array} from the host rows ``block`` (numpy float64 [rows, sum of widths], as ``pack`` laid them out) with the dtype and
    shape ``columns`` (a ``layout``) gives every name; float64 columns are views of ``block``."""
    out, c0 = {}, 0
    for name, tail, dtype, squeeze in columns:
        w = math.prod(tail)
        v = block[:, c0:c0 + w]
        v = v != 0 if dtype == np.bool_ else v.astype(dtype, copy=False)
        out[name] = v[:, 0] if w == 1 and squeeze else v.reshape((block.shape[0],) + tail)
        c0 += w
    return out


# ---- the run ------------------------------------------------------------------------------------------------------------------------

@dataclass
class SurveyRun:
    """One call of survey.infer on one rank: what every block needs, and what the blocks leave behind."""
    ds: object                          # the selected soundings (FdemData / TdemData / TempestData)
    o: dict                             # the options
    common: dict                        # sampler_arguments()
    rows: np.ndarray                    # the selection's rows of the data file (contiguous)
    n_file: int                         # soundings of the data file (replicate c of the sounding in row r: chain r + c n_file)
    rank: int
    C_rep: int                          # replicate chains per sounding
    time_domain: bool
    hitmap: bool
    exact_jacobian: bool
    check_every: int
    results_directory: object           # None: no containers
    container: object                   # "hdf5" | "npz" | None
    own_containers: bool                # this rank fills the containers of its own blocks (one process, or schedule "lines")
    unit_z: object                      # [soundings, M, 2] bounds of the sampled units, or None
    clock: PhaseClock
    # what the blocks leave behind
    dc: object = None                   # the last block's sampler (referenced until infer returns)
    named: tuple = None                 # layout() of its summaries, which is that of every block's result rows
    iterations: int = 0                 # the largest iteration count of any block
    shipped: list = field(default_factory=list)     # per block: payload() on the HOST, for the rank that writes (not own_containers)
    ensemble_diagnostics: object = None     # None, or dict(max_lag): the chain diagnostics of the ensemble join the summaries
    ensemble_correlation: object = None     # None, or dict(band, threshold, keep_band): the resolution length (and the band) join them
    ensemble_families: object = None        # None, or dict(max_families, max_models, measure, min_silhouette): the model families join them
    ensemble_rank_diagnostics: object = None    # None, or dict(max_lag, percentiles): the rank diagnostics of the ensemble join them

    def run_block(self, idx, offset=None, key_by_row=True):
        """Chains of the soundings ``idx`` (rows of ds, ascending) to completion -> (sampler, its ``summaries``).  ``key_by_row``:
        every chain is keyed by its own row of the data file (a selection of the shard); False: ``idx`` is the whole shard, keyed by
        its first row (``common["first_chain"]``)."""
        ds, o, C_rep, clock = self.ds, self.o, self.C_rep, self.clock
        row0 = int(self.rows[0])
        kw = dict(self.common)
        if C_rep > 1:                               # C rows per sounding, sounding-major; every chain keyed by (row of the file, replicate)
            from .replicates import Pooled, expand
            if idx.size:
                rep_rows, chain_id = expand(row0 + idx, C_rep, self.n_file)
                idx = rep_rows - row0
                kw.pop("first_chain")
                kw["chain_id"] = chain_id
        elif key_by_row:
            kw.pop("first_chain")
            kw["chain_id"] = row0 + idx
        if self.unit_z is not None:
            kw["units"] = self.unit_z[idx]           # (with replicates: the expanded rows)
        if self.time_domain:
            from .tdem import TdemDeviceChains
            if isinstance(ds, TempestData):
                # Tempest_datapoint (data/datapoint/Tempest_datapoint.py:106-123, 161-176): the channels hold primary + secondary
                # field, the options file's additive errors are per channel and the sampled level is their multiplier per component
                nc = ds.system[0].n_components
                kw.update(channel_additive=np.asarray(o["initial_additive_error"], dtype=np.float64), initial_additive_error=[1.0] * nc,
                          primary_field=ds.primary_field[idx] if ds.primary_field is not None else None)
            dc = TdemDeviceChains(ds.system, ds.z[idx], ds.total_field(idx) if isinstance(ds, TempestData) else ds.data[idx], offset,
                                  attitude=ds.attitude[idx] if idx.size else None, **kw)
        else:
            from .rjmcmc_gpu import DeviceChains
            with clock.phase("upload_and_initialise"):
                dc = DeviceChains(ds.system, ds.z[idx], ds.data[idx], exact_jacobian=self.exact_jacobian, **kw)
        with clock.phase("chains"):
            dc.infer(check_every=self.check_every)
        diag = None
        if C_rep > 1:
            with clock.phase("pool_replicates"):
                dc = Pooled(dc, C_rep)
                diag = dc.diagnostics()
        return dc, self.summaries(dc, diag)

    def summaries(self, dc, diag=None):
        """The per-sounding summaries of a finished block: [Entry] in the order of the result rows, every tensor as it stands on the device
        (``diag``: Pooled.diagnostics() of a block with replicate chains); an error posterior is [rows, groups, cells] with more than one group."""
        clock = self.clock
        E, i64, f64 = Entry, np.int64, np.float64
        t = dc.t
        named = [E("status", t["status"]), E("burned_in_iteration", t["burned_in_iteration"]), E("n_accepted", t["n_accepted"]),
                 E("misfit", t["misfit"]), E("relative_error", t["rel"]), E("additive_error", t["add"]), E("n_layers", t["k"]),
                 E("best_n_layers", t["best_k"]), E("best_posterior", t["best_posterior"]), E("best_edges", t["best_edges"]),
                 E("best_conductivity", t["best_sigma"]), E("layer_count_posterior", t["k_hist"], i64),
                 E("interface_posterior", t["edge_hist"], i64), E("relative_error_posterior", t["rel_hist"].squeeze(1), i64),
                 E("additive_error_posterior", t["add_hist"].squeeze(1), i64)]
        if getattr(dc, "_moves", None):            # sampled attitude angles (the loops' own convention): final, highest-posterior, posterior
            cur, best = dc.sampled_angles("geom"), dc.sampled_angles("best_geom")
            for q, m_ in enumerate(dc._moves):
                named += [E(m_[0], cur[m_[0]]), E("best_" + m_[0], best[m_[0]]), E(m_[0] + "_posterior", t["geom_hist"][:, q, :m_[5]], i64)]
        if getattr(dc, "solve_height", False):     # the sampled height: final and highest-posterior values, posterior on the prior's 99 cells
            named += [E("height", t["height"]), E("best_height", t["best_height"]), E("height_posterior", t["height_hist"], i64)]
        if self.hitmap:
            with clock.phase("hitmap_statistics"):
                mean, pct = _hitmap_statistics(dc.hitmap, t["log_mean_prior"], dc.value_half_width)     # (attribute access settles dwell times)
            named += [E("mean_log10_conductivity", mean)] + [E("log10_conductivity_" + q, p) for q, p in zip(("p05", "p50", "p95"), pct)]
        if t.get("unit_hist") is not None or t.get("first_hist") is not None:
            from . import unit_posteriors
            with clock.phase("unit_posteriors"):
                named += [E(k_, v_, f64) for k_, v_ in unit_posteriors.products(dc).items()]
        if t.get("data_hist") is not None:
            from . import data_posteriors
            with clock.phase("data_posteriors"):
                named += [E(k_, v_, f64) for k_, v_ in data_posteriors.products(dc).items()]
        if t.get("ens_k") is not None:             # [rows, slots] and [rows, slots, K]; with replicates the chains' slots one after the other
            from . import ensembles
            with clock.phase("ensemble"):
                ens = ensembles.from_chains(dc)
                named += [E("ensemble_k", ens.k, keep=True), E("ensemble_edges", ens.edges, keep=True), E("ensemble_sigma", ens.sigma, keep=True),
                          E("ensemble_misfit", ens.misfit, keep=True), E("ensemble_thin", torch.full_like(t["k"], ens.thin))]
                if self.ensemble_diagnostics is not None:
                    d = ensembles.diagnostics(ens, np.arange(int(dc.n_depth_bins) + 1) * float(dc.depth_bin_width), chains=self.C_rep,
                                              max_lag=self.ensemble_diagnostics["max_lag"])
                    named += [E("ensemble_" + k_, d[k_]) for k_ in ("ess", "rhat", "tau_iterations", "mcse", "ess_k", "ess_misfit", "rhat_k", "rhat_misfit", "ess_min")]
                if self.ensemble_rank_diagnostics is not None:
                    er = self.ensemble_rank_diagnostics
                    d = ensembles.rank_diagnostics(ens, np.arange(int(dc.n_depth_bins) + 1) * float(dc.depth_bin_width), chains=self.C_rep,
                                                   max_lag=er["max_lag"], percentiles=er["percentiles"])
                    named += [E("ensemble_" + k_ + s_, d[k_ + s_]) for s_ in ("", "_k", "_misfit") for k_ in ("rhat_rank", "ess_bulk", "ess_tail")]
                    named += [E("ensemble_ess_bulk_min", d["ess_bulk_min"])]
                if self.ensemble_correlation is not None:
                    ec = self.ensemble_correlation
                    d = ensembles.correlation(ens, np.arange(int(dc.n_depth_bins) + 1) * float(dc.depth_bin_width), chains=self.C_rep,
                                              band=ec["band"], threshold=ec["threshold"], keep_band=ec["keep_band"])
                    named += [E("ensemble_" + k_, d[k_], keep=True) for k_ in ("resolution_length", "resolution_cells", "resolution_closed")]
                    if ec["keep_band"]:
                        named += [E("ensemble_correlation_band", d["band"], keep=True)]
                if self.ensemble_families is not None:
                    from . import families
                    ef = self.ensemble_families
                    d = families.families(ens, float(int(dc.n_depth_bins) * float(dc.depth_bin_width)), z0=0.0, measure=ef["measure"],
                                          chains=self.C_rep, max_families=ef["max_families"], max_models=ef["max_models"],
                                          min_silhouette=ef["min_silhouette"])
                    named += [E("ensemble_families_n", d["n_families"]), E("ensemble_family_share", d["family_share"], keep=True),
                              E("ensemble_family_silhouette", d["silhouette"], keep=True), E("ensemble_family_k", d["family_k"], keep=True),
                              E("ensemble_family_edges", d["family_edges"], keep=True), E("ensemble_family_sigma", d["family_sigma"], keep=True),
                              E("ensemble_central_k", d["central_k"]), E("ensemble_central_edges", d["central_edges"], keep=True),
                              E("ensemble_central_sigma", d["central_sigma"], keep=True),
                              E("ensemble_central_mean_distance", d["central_mean_distance"])]
        if diag is not None:
            named += [E(k_, diag[k_], i64 if k_ == "n_used" else f64, k_ == "chain_mean") for k_ in REPLICATE_SUMMARIES] + [E("replicates_used", dc.use.sum(dim=1))]
        return named

    def payload(self, dc, idx, sparse=False):
        """The rows of hdf.device_row_fields for a finished block, moved to host memory at once (the hit maps are 440 KB per
        sounding: what stays on the GPU is the running block, not every block a rank has finished) -> (rows, float64 rows, int32
        rows[, (ptr, index, value)]).  ``sparse``: the hit maps leave the device in run-length form (per row: the flat positions
        value_bin * n_depth + depth cell at which the count changes, and the counts; hdf._Dataset.write_run_rows) instead of dense
        int32 columns -- depth is the fast axis and a layer fills a run of cells with one count: a few thousand runs against 110 000
        cells -- for a process that fills its own containers.  The columns stand in the order survey._row_fields gives, which is the
        order _LineWriter reads them in."""
        from .rjmcmc_gpu import layer_widths
        ds = self.ds
        t, dev = dc.t, dc.device
        n_mc = int(self.o["n_markov_chains"])
        none = t["best_k"] < 1                      # (a chain that never recorded a best model: its current one)
        bk = torch.where(none, t["k"], t["best_k"])
        be = torch.where(none[:, None], t["edges"], t["best_edges"])
        bs = torch.where(none[:, None], t["sigma"], t["best_sigma"])
        # the error levels of the highest-posterior state, like Inference1D.writeHdf's best data point (:1076-1088)
        brel = torch.where(none[:, None], t["rel"], t["best_rel"]).contiguous()
        badd = torch.where(none[:, None], t["add"], t["best_add"]).contiguous()
        observed = dc.observed                     # (the measured data: t["data"] unless the chains sampled the prior alone)
        pred = torch.empty_like(observed)
        chi2, logl = torch.empty_like(t["misfit"]), torch.empty_like(t["misfit"])
        # sampled attitude angles: the best data point's OWN geometry -- the prediction and the predicted primary field of the
        # highest-posterior angles, not of the chain's last state / the measured geometry (Inference1D.writeHdf :1076-1088 writes
        # the best data point: predicted_secondary_field = predictedData - predicted_primary_field there)
        best_mix = {}
        best_primary = None
        eval_height = t["best_height"] if t.get("best_height") is not None else t["height"]
        moves = getattr(dc, "_moves", None) or ()
        if moves:
            bw, boff, best_primary = dc.mix_for_geometry(torch.where(none[:, None], t["geom"], t["best_geom"]))
            best_mix = dict(weights=bw, offset=boff)
            extra = dc.geometry_rows_extra()       # sampled positions: the best state's distance scale and effective height
            if extra is not None:
                best_mix["scale"], eval_height = extra["scale"], extra["height"]
        with torch.cuda.device(dev):                # one batched forward at the best models, through the sampler's own entry
            dc._eval_loglike(bk.contiguous(), bs.contiguous(), layer_widths(be, bk.to(torch.int64)).contiguous(),
                             eval_height, observed, brel, badd, pred, chi2, logl, **best_mix)
        host = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)[idx], device=dev).reshape(idx.size, -1)
        F = dict(x=host(ds.x), y=host(ds.y), z=host(ds.z), elevation=host(ds.elevation), line_number=host(ds.lineNumber),
                 fiducial=host(ds.fiducial), data=observed, predicted=pred, relative_error=brel, additive_error=badd,
                 log_mean_prior=t["log_mean_prior"][:, None], best_edges=be, best_sigma=bs)
        st, bi = t["status"].to(torch.int32), t["burned_in_iteration"].to(torch.int32)
        ran = torch.where(st == 1, bi + n_mc + 1, torch.where(st == 2, torch.full_like(bi, n_mc), torch.full_like(bi, dc.iteration)))
        I = dict(status=st[:, None], burned_in_iteration=bi[:, None], iterations=ran[:, None], best_k=bk[:, None],
                 best_iteration=t["best_iteration"][:, None], k_hist=t["k_hist"], edge_hist=t["edge_hist"], rel_hist=t["rel_hist"].flatten(1),
                 add_hist=t["add_hist"].flatten(1))
        if self.time_domain:
            F.update(std=dc.channel_std(observed, brel, badd), offset=host(ds.offsets), loop_angles=host(ds.loop_angles))
            if ds.primary_field is not None and ds.primary_field.shape[1]:
                F.update(primary=host(ds.primary_field),
                         predicted_primary=torch.as_tensor(dc.predicted_primary() if best_primary is None else best_primary, device=dev).reshape(idx.size, -1))
        if getattr(dc, "solve_height", False):
            F.update(best_height=t["best_height"][:, None], height0=t["height0"][:, None])
            I.update(height_hist=t["height_hist"])
        if moves:
            bst, ctr = dc.sampled_angles("best_geom"), dc.sampled_angles("geom0")
            for q_, m_ in enumerate(moves):
                F.update({"best_" + m_[0]: bst[m_[0]][:, None], m_[0] + "_centre": ctr[m_[0]][:, None]})
                I[m_[0] + "_hist"] = t["geom_hist"][:, q_, :m_[5]]
        if getattr(dc, "trace_every", 0):
            F.update(trace_misfit=t["trace_misfit"])
            I.update(trace_accept=t["trace_accept"])
        layout_f, layout_i, _ = _row_fields(ds, dc, self.hitmap and not sparse)
        f64_block = pack_rows(F, layout_f)
        csr = None
        if self.hitmap and sparse:
            from .hitmap import runs                # run starts: a row's first cell and every change of value (csrc/gbp_hitmap.h)
            ptr, start_, val_ = runs(dc.hitmap)     # (attribute access settles the dwell times)
            csr = (ptr.cpu().numpy(), start_.cpu().numpy(), val_.cpu().numpy())
            del start_, val_
        elif self.hitmap:
            I.update(hitmap=dc.hitmap.flatten(1))   # (attribute access settles the dwell times)
        out = (torch.as_tensor(np.asarray(idx), dtype=torch.int64), f64_block.cpu(), pack_rows(I, layout_i, torch.int32).cpu())
        return out + (csr,) if sparse else out

    def process(self, first, count, filler, key_by_row=True):
        """Result rows [count, width] of the soundings first .. first + count - 1 (count >= 0): one block.  The block before it, if
        ``filler`` holds one, leaves the device while this block's chains run."""
        ds = self.ds
        span = np.arange(first, first + count)
        offset = None
        if self.time_domain:
            # the Hankel tables depend on the horizontal transmitter-receiver distance and dz: the block's handle holds one table
            # set per distinct pair and every chain runs with its own; azimuth and attitude are per-chain mixing weights
            # (TdemDeviceChains(offset=[n, 3], attitude=[n, 6])) -- one block whatever the geometry
            n_off = np.unique(np.c_[np.hypot(ds.offsets[span, 0], ds.offsets[span, 1]), ds.offsets[span, 2]], axis=0).shape[0] if count > 0 else 1
            if n_off > TdemData.MAX_OFFSET_SETS:
                raise NotImplementedError("{} distinct (horizontal distance, dz) receiver offsets in {} soundings: the device sampler holds one "
                                          "set of Hankel tables (~0.15 MB x (1 + altitude bins)) per pair -- bin the offsets (e.g. to 0.1 m) first".format(n_off, count))
            offset = ds.offsets[span] if count > 0 else (0.0, 0.0, 0.0)
        filler.drain(background=True)
        dc, entries = self.run_block(span, offset, key_by_row)
        if self.own_containers:
            # the block's rows go to the line containers and are dropped (host memory holds the open lines, not the survey's hit
            # maps) -- at the start of the next block, or, for the last one, once the summary file's thread is running
            filler.hand_over(dc, span)
        elif self.results_directory is not None and span.size:      # (a rank that drew no chunk ships nothing)
            self.shipped.append(self.payload(dc, span))
        columns = layout(entries)
        if self.named is not None and self.named != columns:
            raise ValueError("result rows: this block's columns are not those of the block before it")
        self.iterations, self.dc, self.named = max(self.iterations, dc.iteration), dc, columns
        return pack(entries)

    def gather_pieces(self, pieces, filler):
        """The blocks ``pieces`` (an iterable of (first, count); every chain keyed by its own row) of this rank, one after the other,
        and the exchange of their result rows -> [soundings, width] on rank 0 (distributed.gather_rows)."""
        from .distributed import gather_rows
        done_rows, done_vals = [], []
        for first, count in pieces:
            done_vals.append(self.process(first, count, filler))
            done_rows.append(torch.arange(first, first + count, dtype=torch.int64, device=done_vals[-1].device))
        if not done_vals:                           # this rank got nothing: an empty block fixes the row width and the device
            done_vals.append(self.process(0, 0, filler))
            done_rows.append(torch.zeros(0, dtype=torch.int64, device=done_vals[-1].device))
        return gather_rows(torch.cat(done_rows), torch.cat(done_vals), self.ds.nPoints)

    def write_containers(self, filler):
        """The end of the results containers: this rank's own (the last block's rows, then the open lines), or every rank's rows to
        rank 0 (_write_line_containers)."""
        if self.own_containers:
            filler.finish(self.dc)
        elif self.results_directory is not None:
            _write_line_containers(self.results_directory, self.ds, self.o, self.dc, self.shipped, self.hitmap, self.rank, self.container)


# ---- the container filler -----------------------------------------------------------------------------------------------------------

class ContainerFiller:
    """Finished blocks -> host -> line containers, one block at a time.  ``hand_over`` takes a finished block; the next ``drain`` moves
    it: in the foreground, or (``background``) on a host thread with a device stream of its own, while the caller's thread runs the
    NEXT block's chains.  The block's sampler stays alive until its rows have left the device; one block is in flight at a time, so the
    writer receives the blocks in order -- 65 536 soundings: the rows of three of the four blocks no longer stand between two blocks'
    chains.  The phase clocks of a background fill are host wall time, overlapped with "chains".

    ``payload(dc, idx)``: the block's rows on the host; ``make_writer(dc)``: the writer (``add_block``, ``finish``), made when the first
    block arrives; ``device_stream`` False: background fills run on a plain thread whatever the device (no stream is made).

    A context manager around the loop over the blocks: on exit the fill thread is joined; what it raised is raised there, or, when the
    body raised, attached to the end of that exception's ``__context__`` chain."""

    def __init__(self, payload, make_writer, clock, device_stream=True):
        self.payload, self.make_writer, self.clock, self.device_stream = payload, make_writer, clock, device_stream
        self.writer = None
        self.unfilled = None            # (sampler, rows) of the block that has not left the device yet
        self.side = None                # the background fills' device stream
        self.thread = None
        self.failed = []                # what the fill thread raised, until the caller's thread has seen it

    def hand_over(self, dc, idx):
        self.unfilled = (dc, idx)

    def _join(self):
        th, self.thread = self.thread, None
        if th is not None:
            th.join()

    def drain(self, background=False):
        self._join()
        if self.failed:
            raise self.failed.pop(0)
        if self.unfilled is None:
            return
        (dc, idx), self.unfilled = self.unfilled, None
        if self.writer is None:
            self.writer = self.make_writer(dc)
        if idx.size == 0:                           # (a rank that got no flight line: nothing to hand over)
            return
        if not background or (self.device_stream and dc.device.type != "cuda"):
            with self.clock.phase("rows_to_host"):
                pl = self.payload(dc, idx)
            with self.clock.phase("container_fill"):
                self.writer.add_block(pl)
            return
        if self.device_stream:
            if self.side is None:
                self.side = torch.cuda.Stream(device=dc.device)
            self.side.wait_stream(torch.cuda.current_stream(dc.device))      # (the block's chains have ended: infer() read their status flags)
        self.thread = threading.Thread(target=self._work, args=(dc, idx))
        self.thread.start()

    def _work(self, dc, idx):
        try:
            t0 = time.perf_counter()
            if self.device_stream:
                with torch.cuda.device(dc.device), torch.cuda.stream(self.side):
                    pl = self.payload(dc, idx)
            else:
                pl = self.payload(dc, idx)
            t1 = time.perf_counter()
            self.writer.add_block(pl)
            self.clock.add("rows_to_host_overlapped", t1 - t0)
            self.clock.add("container_fill_overlapped", time.perf_counter() - t1)
        except BaseException as e:                   # (handed to the caller's thread by drain / __exit__)
            self.failed.append(e)

    def finish(self, dc):
        """The last block in the foreground, then the writer's own end (``dc``: the sampler an empty set of containers is made from
        when there was no sounding at all)."""
        self.drain()
        if self.writer is None:
            self.writer = self.make_writer(dc)
        with self.clock.phase("compress_and_write_tail"):
            return self.writer.finish()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self._join()
        if not self.failed:
            return False
        fill_error = self.failed.pop(0)
        if exc is None:
            raise fill_error
        tail = exc
        while tail.__context__ is not None and tail.__context__ is not fill_error:
            tail = tail.__context__
        tail.__context__ = fill_error
        return False


# ---- the result ---------------------------------------------------------------------------------------------------------------------

def assemble_result(ds, o, dc, columns, r, iterations_run):
    """The SurveyResult from the gathered result rows ``r`` (numpy [soundings, width], laid out as ``columns``: SurveyRun.named; ``dc``:
    any block's sampler, for the depth axis; ``iterations_run``: the count of a chain that never finished)."""
    res = SurveyResult(line=ds.lineNumber, fiducial=ds.fiducial, x=ds.x, y=ds.y, z=ds.z, elevation=ds.elevation,
                       depth_bin_width=np.float64(dc.depth_bin_width))
    res.update(unpack(columns, r))
    n_mc = int(o["n_markov_chains"])             # iterations each chain ran before it froze
    ran = np.where(res["status"] == 1, res["burned_in_iteration"] + n_mc + 1, np.where(res["status"] == 2, n_mc, iterations_run))
    res["iterations"] = ran.astype(np.int64)
    res["acceptance"] = res.pop("n_accepted") / np.maximum(1, ran)
    return res
