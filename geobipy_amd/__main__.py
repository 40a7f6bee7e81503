"""Command line of the survey driver: ``python -m geobipy_amd options_file output_directory [...]``.

Same positional arguments and switches as the reference's ``geobipy`` command (geobipy/__init__.py:76-243).  Instead of
``--mpi`` under mpirun, launch one process per GPU with ``python -m torch.distributed.run --nproc-per-node N -m geobipy_amd
...``: each rank takes a block of soundings and rank 0 writes the results, one ``<line number>.npz`` per flight line.
"""
import argparse
import os
import shutil
import sys
import time


def parse(argv=None):
    p = argparse.ArgumentParser(prog="geobipy_amd", description="GeoBIPy's rjMCMC inversion of FDEM soundings on MI355X GPUs",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("options_file", help="User options file")
    p.add_argument("output_directory", help="Output directory for results")
    p.add_argument("--seed", dest="seed", default=None, help="Seed of the random streams (overrides the options file)")
    p.add_argument("--index", dest="index", type=int, default=None, help="Invert this data point only.")
    p.add_argument("--fiducial", dest="fiducial", type=float, default=None, help="Invert this fiducial only (needs --line).")
    p.add_argument("--line", dest="line_number", type=float, default=None, help="Invert this line (or the fiducial on this line).")
    p.add_argument("--verbose", dest="verbose", action="store_true", help="Throw warnings as errors.")
    p.add_argument("--mpi", dest="mpi", action="store_true", help="Accepted for compatibility: ranks come from torch.distributed.run.")
    p.add_argument("--data_directory", default=None, help="override data_directory in parameter file.")
    p.add_argument("--data_filename", default=None, help="override data_filename in parameter file")
    p.add_argument("--exact-jacobian", action="store_true", help="true derivative in the proposals (DESIGN.md 3.4)")
    p.add_argument("--no-hitmap", action="store_true", help="skip the conductivity-depth hit map")
    p.add_argument("--hankel-eps", type=float, default=None,
                   help="accuracy budget of the Hankel-filter abscissa window: ppm for frequency-domain data (default 1e-10, 0 = all "
                        "abscissae), relative to the inductive-limit value for time-domain data (default 1e-12)")
    p.add_argument("--no-containers", action="store_true",
                   help="skip the reference-layout results containers (<line>.h5 -- real HDF5, through h5py or the HDF5 C library -- or, where neither "
                        "exists, the stand-in <line>.results.npz + <line>.results.attrs.json with the same dataset paths); the per-line "
                        "summary files <line>.npz are always written")
    p.add_argument("--container", choices=("auto", "hdf5", "npz"), default="auto",
                   help="file type of the results containers: hdf5 (<line>.h5), npz (the stand-in), auto = hdf5 when it can be written")
    p.add_argument("--schedule", choices=("auto", "static", "dynamic", "lines"), default="auto",
                   help="lines: whole flight lines per rank, each rank writes the results containers of its own lines and only the "
                        "one-row summaries travel (one all_gather_into_tensor: the exchange that has run under RCCL); static: one "
                        "contiguous block of soundings per rank; dynamic: ranks draw chunks from a shared counter (the reference's "
                        "master / worker scheduling) and ship their posterior rows to rank 0 point to point (tested over gloo only); "
                        "auto = lines on more than one rank when every flight line is one run of rows of the data file, else static")
    p.add_argument("--chunk", type=int, default=None, help="soundings per block on the device (default: 16384 for static and lines, fewer when full-length traces would not fit the device budget; a 16th of a rank's share for dynamic)")
    p.add_argument("--traces", default="1",
                   help="per-iteration misfit / acceptance traces of the containers: 1 = the reference's arrays in full (2 n_markov_chains "
                        "columns), an integer stride > 1 or 'auto' (at most 4096 entries per sounding) keeps every stride-th entry, 0 = none")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--units-depth", type=float, nargs="+", default=None, metavar="E",
                   help="sampled unit posteriors (conductance, transverse resistance: unit_* in the summaries) of the units between these depths, m")
    g.add_argument("--units-elevation", type=float, nargs="+", default=None, metavar="E",
                   help="the same for the units between these elevations (m) under each sounding's surface")
    p.add_argument("--unit-kinds", nargs="+", choices=("arithmetic", "harmonic"), default=["arithmetic", "harmonic"],
                   help="unit means to accumulate (default both)")
    p.add_argument("--first-above", type=float, nargs="+", default=[], metavar="S",
                   help="posterior of the depth to the first layer at or above these conductivities, S/m (first_depth_* in the summaries)")
    p.add_argument("--first-below", type=float, nargs="+", default=[], metavar="S", help="... at or below these conductivities, S/m")
    p.add_argument("--replicates", type=int, default=1, metavar="C",
                   help="chains per sounding, 1 .. 8 (frequency-domain data): the posteriors are pooled over the chains that burned in and the "
                        "summaries gain per-depth-cell convergence maps (rhat, jsd, n_used, ...)")
    p.add_argument("--data-posteriors", type=int, nargs="?", const=64, default=None, metavar="N_BINS",
                   help="data-space posteriors (residual of every channel's prediction, misfit: data_* / misfit_* in the summaries) on "
                        "N_BINS cells (8 .. 256, default 64)")
    p.add_argument("--ensemble", type=int, nargs="*", default=None, metavar="N",
                   help="keep a posterior ensemble: N_KEEP [THIN] -- every THIN-th sampled model of every sounding, up to N_KEEP (1 .. 4096, "
                        "default 64; THIN defaults to ceil(n_markov_chains / N_KEEP)): ensemble_* in the summaries")
    p.add_argument("--ensemble-diagnostics", type=int, nargs="?", const=255, default=None, metavar="MAX_LAG",
                   help="chain diagnostics of the ensemble (needs --ensemble): effective sample size, split R-hat, autocorrelation time and "
                        "Monte-Carlo standard error per depth cell, lags up to MAX_LAG (1 .. 255, default 255): ensemble_ess, ensemble_rhat, "
                        "... in the summaries")
    p.add_argument("--ensemble-rank-diagnostics", type=int, nargs="?", const=255, default=None, metavar="MAX_LAG",
                   help="rank diagnostics of the ensemble (needs --ensemble): rank-normalised and folded split R-hat, bulk and tail "
                        "effective sample size per depth cell, lags up to MAX_LAG (1 .. 255, default 255): ensemble_rhat_rank, "
                        "ensemble_ess_bulk, ensemble_ess_tail, ... in the summaries")
    p.add_argument("--ensemble-correlation", nargs="*", default=None, metavar="BAND [THRESHOLD]",
                   help="vertical resolution from the ensemble (needs --ensemble): the posterior correlation between depth cells up to BAND "
                        "cells apart (>= 0, default 64) and the thickness over which it stays >= THRESHOLD (0 < THRESHOLD < 1, default 0.5): "
                        "ensemble_resolution_length, ensemble_resolution_cells, ensemble_resolution_closed in the summaries")
    p.add_argument("--ensemble-families", type=int, nargs="?", const=4, default=None, metavar="QMAX",
                   help="model families from the ensemble (needs --ensemble): the representative (medoid) model of every sounding and up to "
                        "QMAX families of kept models (1 .. 8, default 4): ensemble_central_*, ensemble_families_n, ensemble_family_* in the "
                        "summaries")
    a = p.parse_args(argv)
    if a.ensemble_correlation is not None:
        if len(a.ensemble_correlation) > 2:
            p.error("--ensemble-correlation: at most BAND and THRESHOLD")
        try:
            a.ensemble_correlation = dict(band=int(a.ensemble_correlation[0]) if a.ensemble_correlation else 64,
                                          threshold=float(a.ensemble_correlation[1]) if len(a.ensemble_correlation) > 1 else 0.5)
        except ValueError:
            p.error("--ensemble-correlation: BAND is an integer, THRESHOLD a number")
    # the ranges, and that each of the four needs --ensemble, are infer's own checks
    from . import survey_run
    try:
        if a.ensemble_families is not None:
            survey_run.ensemble_families_argument(dict(max_families=a.ensemble_families), a.ensemble)
        if a.ensemble_correlation is not None:
            survey_run.ensemble_correlation_argument(a.ensemble_correlation, a.ensemble)
        if a.ensemble_diagnostics is not None:
            survey_run.ensemble_diagnostics_argument(dict(max_lag=a.ensemble_diagnostics), a.ensemble)
        if a.ensemble_rank_diagnostics is not None:
            survey_run.ensemble_rank_diagnostics_argument(dict(max_lag=a.ensemble_rank_diagnostics), a.ensemble)
    except ValueError as e:
        p.error(str(e))
    if a.ensemble is not None:
        if len(a.ensemble) > 2:
            p.error("--ensemble: at most N_KEEP and THIN")
        a.ensemble = dict(n_keep=a.ensemble[0] if a.ensemble else 64, thin=a.ensemble[1] if len(a.ensemble) > 1 else None)
        if not 1 <= a.ensemble["n_keep"] <= 4096 or (a.ensemble["thin"] is not None and a.ensemble["thin"] < 1):
            p.error("--ensemble: N_KEEP in 1 .. 4096, THIN >= 1")
        if a.no_hitmap:
            p.error("--ensemble needs the hit map (drop --no-hitmap)")
    if a.data_posteriors is not None:
        if not 8 <= a.data_posteriors <= 256:
            p.error("--data-posteriors: 8 .. 256 cells")
        if a.no_hitmap:
            p.error("--data-posteriors needs the hit map (drop --no-hitmap)")
    if not 1 <= a.replicates <= 8:
        p.error("--replicates: 1 .. 8 chains per sounding")
    if a.replicates > 1 and a.no_hitmap:
        p.error("--replicates needs the hit map (drop --no-hitmap)")
    a.units = None
    if a.units_depth is not None or a.units_elevation is not None:
        from .intervals import edges_argument
        try:
            a.units = (dict(kind="depth", edges=edges_argument(a.units_depth)) if a.units_depth is not None
                       else dict(kind="elevation", edges=edges_argument(a.units_elevation)))
        except ValueError as e:
            p.error(str(e))
    if len(a.first_above) + len(a.first_below) > 4 or any(not (v > 0.0 and v < float("inf")) for v in a.first_above + a.first_below):
        p.error("--first-above / --first-below: at most 4 thresholds in all, each finite and positive (S/m)")
    if (a.units is not None or a.first_above or a.first_below) and a.no_hitmap:
        p.error("--units-* / --first-* need the hit map (drop --no-hitmap)")
    a.traces = "auto" if a.traces == "auto" else (int(a.traces) or None)
    if a.seed is not None:
        a.seed = int(a.seed)
    return a


def main(argv=None):
    a = parse(argv)
    if a.verbose:
        import warnings
        warnings.filterwarnings("error")
    assert os.path.exists(a.options_file), Exception("Cannot find input file {}".format(a.options_file))
    assert os.path.isdir(a.output_directory), Exception("Make sure the output directory exists {}".format(a.output_directory))
    import torch
    import torch.distributed as dist
    from . import survey
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(os.environ.get("GBP_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
    if rank == 0:
        print("Running geobipy_amd on {} GPU process(es)".format(world))
        print("Using user input file {}".format(a.options_file))
        print("Output files will be produced at {}".format(a.output_directory))
        shutil.copy(a.options_file, a.output_directory)            # kept with the results, like the reference does
    containers = None if a.no_containers else a.output_directory      # reference-layout containers: FdemData, TdemData, TempestData
    t0 = time.perf_counter()
    res = survey.infer(a.options_file, seed=a.seed, index=a.index, fiducial=a.fiducial, line_number=a.line_number,
                       exact_jacobian=a.exact_jacobian, hitmap=not a.no_hitmap, hankel_eps=a.hankel_eps, schedule=a.schedule, chunk=a.chunk, traces=a.traces, results_directory=containers,
                       container=None if a.container == "auto" else a.container, data_directory=a.data_directory,
                       data_filename=a.data_filename, units=a.units, unit_kinds=tuple(a.unit_kinds), first_above=tuple(a.first_above),
                       first_below=tuple(a.first_below), replicates=a.replicates,
                       data_posteriors=None if a.data_posteriors is None else dict(n_bins=a.data_posteriors), ensemble=a.ensemble,
                       ensemble_diagnostics=False if a.ensemble_diagnostics is None else dict(max_lag=a.ensemble_diagnostics),
                       ensemble_correlation=False if a.ensemble_correlation is None else a.ensemble_correlation,
                       ensemble_families=False if a.ensemble_families is None else dict(max_families=a.ensemble_families),
                       ensemble_rank_diagnostics=False if a.ensemble_rank_diagnostics is None else dict(max_lag=a.ensemble_rank_diagnostics))
    if rank == 0:
        paths = res.save_lines(a.output_directory)
        done, failed = int((res["status"] == 1).sum()), int((res["status"] == 2).sum())
        print("{} soundings: {} done, {} failed to burn in; {:.1f} s; wrote {}".format(
            res["status"].size, done, failed, time.perf_counter() - t0, ", ".join(os.path.basename(q) for q in paths)))
        if containers is not None:
            from . import hdf
            kind = hdf.container_type(None if a.container == "auto" else a.container)
            print("results containers (the reference's Inference2D / Inference1D layout): " +
                  ("HDF5 files <line>.h5, written by " + str(hdf.hdf5_writer()) if kind == "hdf5" else
                   "written as the stand-in <line>.results.npz + <line>.results.attrs.json (same dataset paths, "
                   "geobipy_amd.hdf.load_npz reads them; NOT HDF5 files -- neither h5py nor a loadable HDF5 library here, or --container npz)"))
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
